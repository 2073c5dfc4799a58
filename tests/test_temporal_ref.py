"""The temporal depth filter's definition, checked on the CPU: tests/temporal_ref.py (numpy int64, the yardstick of temporal.hip) against a
plain-Python per-pixel loop on every hand-made case; the mutants the cases kill; the consequences include/NativeUtils.h states; a call of n
ticks against n calls of one tick; and the branch mix of the fuzz tests' seeded inputs."""
import itertools

import numpy as np
import pytest

from tests import temporal_cases as cases, temporal_ref as ref

CASES = cases.cases()


def _loop(maps, state, alpha_q, delta, persist):
    outs, brs = np.zeros(maps.shape, np.uint16), np.zeros(maps.shape, np.uint8)
    words = [int(x) for x in state]
    for t in range(maps.shape[0]):
        for i in range(maps.shape[1]):
            outs[t, i], words[i], brs[t, i] = ref.pixel(int(maps[t, i]), words[i], alpha_q, delta, persist)
    return outs, np.array(words, dtype=np.uint32), brs


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_restatement_equals_the_plain_loop_and_the_case_reaches_its_boundary(case):
    out, state, br = case.want()
    lo, ls, lb = _loop(case.maps, case.state, *case.params)
    assert np.array_equal(out, lo) and np.array_equal(state, ls) and np.array_equal(br, lb)
    assert ref.state_ok(case.state) and ref.state_ok(state)
    case.witness()


def test_the_cases_name_what_the_issue_lists():
    names = {c.name for c in CASES}
    assert {"gate_delta_1", "gate_delta_20", "gate_delta_4095", "alpha_1", "alpha_255", "alpha_256", "rounding_floor_and_half", "stall",
            "extremes_of_F_and_c", "persist_0", "persist_1", "persist_255", "miss_254_255_then_expires", "hole_without_history",
            "sample_returns_after_a_fill", "gate_failure_then_reblend"} <= names
    assert len(names) == len(CASES)


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_every_mutant_is_killed_by_a_case(mutant):
    killers = []
    for c in CASES:
        out, state, _ = c.want()
        mo, ms, _ = c.want(mutant)
        if not (np.array_equal(out, mo) and np.array_equal(state, ms)):
            killers.append(c.name)
    assert killers, mutant


def test_consequences_over_the_extremes_of_the_parameters():
    """F' of a blend between F and 256 c and the served value in [1, 65535] (temporal_ref.step asserts both on every call), the state
    stays admissible, alpha_q = 256 with persist = 0 is the identity on the maps -- over every extreme of the parameters, on states and
    samples at and around every boundary."""
    F = np.array([0, 256, 257, 383, 384, 256 * 1000 - 1, 256 * 1000, 256 * 1000 + 128, 65535 * 256 - 1, 65535 * 256], dtype=np.int64)
    c = np.array([0, 1, 2, 999, 1000, 1001, 1020, 5095, 65534, 65535], dtype=np.int64)
    for alpha, delta, persist in itertools.product((1, 2, 127, 128, 255, 256), (1, 20, 4095), (0, 1, 254, 255)):
        for miss in (0, 1, 253, 254, 255):
            FF, cc = np.meshgrid(F, c)
            state = ref.pack(FF.ravel(), np.where(FF.ravel() == 0, 0, miss))
            out, s2, br = ref.step(cc.ravel(), state, alpha, delta, persist)
            assert ref.state_ok(s2)
            lo = [ref.pixel(int(x), int(w), alpha, delta, persist) for x, w in zip(cc.ravel(), state)]
            assert out.tolist() == [p[0] for p in lo] and s2.tolist() == [p[1] for p in lo] and br.tolist() == [p[2] for p in lo]
            if alpha == 256 and persist == 0:
                assert np.array_equal(out, cc.ravel())


def test_identity_setting_on_a_sequence():
    _, _, maps = cases.fuzz_case(0)
    out, state, _ = ref.run(maps, np.zeros(maps.shape[1], np.uint32), 256, 20, 0)
    assert np.array_equal(out, maps)
    assert np.array_equal(state, maps[-1].astype(np.uint32) * 256)


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS[:4])
def test_n_ticks_in_one_call_equal_n_calls_of_one_tick(seed):
    _, params, maps = cases.fuzz_case(seed)
    zero = np.zeros(maps.shape[1], np.uint32)
    out, state, br = ref.run(maps, zero, *params)
    s, outs = zero, []
    for t in range(maps.shape[0]):
        o, s, _ = ref.run(maps[t:t + 1], s, *params)
        outs.append(o[0])
    assert np.array_equal(out, np.stack(outs)) and np.array_equal(state, s)
    k = maps.shape[0] // 2
    o1, s1, _ = ref.run(maps[:k], zero, *params)
    o2, s2, _ = ref.run(maps[k:], s1, *params)
    assert np.array_equal(out, np.concatenate([o1, o2])) and np.array_equal(state, s2)


def test_lag_is_by_design():
    """A surface that moves by less than delta per tick is blended every tick and lags behind itself."""
    maps = (1000 + 5 * np.arange(24, dtype=np.int64)).astype(np.uint16).reshape(-1, 1)
    out, _, br = ref.run(maps, np.zeros(1, np.uint32), 64, 20, 0)
    assert (br[1:] == ref.BLEND).all() and (out[1:] < maps[1:]).all() and out[-1, 0] <= maps[-1, 0] - 10


def test_fuzz_inputs_take_every_branch():
    """Over the fuzz tests' seeded inputs each of the six branches takes at least 2 % of all pixel-ticks."""
    total = np.zeros(6, dtype=np.int64)
    for seed in cases.FUZZ_SEEDS:
        _, params, maps = cases.fuzz_case(seed)
        _, _, br = ref.run(maps, np.zeros(maps.shape[1], np.uint32), *params)
        total += np.bincount(br.ravel(), minlength=6)
    share = total / total.sum()
    print({name: round(float(s), 4) for name, s in zip(ref.BRANCHES, share)})
    assert (share >= 0.02).all(), dict(zip(ref.BRANCHES, share.tolist()))
    assert {cases.fuzz_case(s)[1][2] for s in cases.FUZZ_SEEDS} == {0, 1, 2}
    assert {1, 256} <= {cases.fuzz_case(s)[1][0] for s in cases.FUZZ_SEEDS} and {1, 4095} <= {cases.fuzz_case(s)[1][1] for s in cases.FUZZ_SEEDS}
