"""The temporal depth filter (temporal.hip: lsnFusionSetTemporal / lsnFusionTemporal / lsnFusionTemporalReset / lsnFusionTemporalStateRead /
lsnFusionTemporalStateWrite / lsnFusionTemporalDiagnostics) on the GPU.

Bar: bit for bit against the numpy restatement (tests/temporal_ref.py), for the maps AND the state; the diagnostics equal the
restatement's branch counts per sensor and tick.  Every map buffer sits between guard bands.  Every test here fails on a library without
the feature (the exports do not exist)."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import temporal_cases as cases, temporal_ref as ref
from tests.support import Guarded

pytestmark = pytest.mark.gpu

SETTING = (64, 20, 2)


class Batch:
    """A plan of `sizes` sensors and T ticks, its input at `shift` bytes behind a 16-byte boundary, input and output between guard bands."""

    def __init__(self, sizes, T, shift=0):
        import torch
        self.torch, self.sizes, self.T = torch, sizes, T
        self.widths, self.heights = [s[0] for s in sizes], [s[1] for s in sizes]
        self.plan = native.FusionPlan(0, T, self.widths, self.heights)
        self.px = self.plan.capacity
        assert self.px == sum(w * h for w, h in sizes)
        self.nbytes = 2 * self.px * T
        self.src = Guarded(torch, self.nbytes + shift, "cuda")
        self.dst = Guarded(torch, self.nbytes + shift, "cuda")
        self.src_ptr, self.dst_ptr, self.shift = self.src.ptr + shift, self.dst.ptr + shift, shift
        self.slices = ref.sensor_slices(self.widths, self.heights)

    def load(self, maps):
        assert maps.shape == (self.T, self.px)
        self.src.body()[self.shift:].copy_(self.torch.from_numpy(np.ascontiguousarray(maps, "<u2").view(np.uint8).ravel().copy()))

    def source(self):
        return self.src.body()[self.shift:].cpu().numpy().view("<u2").reshape(self.T, self.px)

    def run(self, in_place=False):
        """-> the filtered maps [T, pixels]."""
        if not in_place:
            self.dst.body().fill_(0x5A)
        self.plan.temporal(self.src_ptr, self.src_ptr if in_place else self.dst_ptr)
        self.torch.cuda.synchronize()
        assert self.dst.intact() and self.src.intact()
        out = self.src if in_place else self.dst
        return out.body()[self.shift:].cpu().numpy().view("<u2").reshape(self.T, self.px)

    def check(self, maps, state, params, what, in_place=False):
        """One call on `maps` from `state` (None: the plan's own): maps, state and diagnostics against the restatement.  -> state'."""
        if state is not None:
            self.plan.set_temporal_state(state)
        before = self.plan.temporal_state()
        self.load(maps)
        want, wstate, br = ref.run(maps, before, *params)
        got = self.run(in_place)
        assert np.array_equal(got, want), (what, int((got != want).sum()))
        gstate = self.plan.temporal_state()
        assert np.array_equal(gstate, wstate), (what, int((gstate != wstate).sum()))
        if not in_place:
            assert np.array_equal(self.source(), maps), what            # the input stays as it was
        for t in range(self.T):
            d = self.plan.temporal_diagnostics(t)
            assert d.tolist() == [list(ref.counts(br[t, s])) for s in self.slices], (what, t)
        return wstate

    def close(self):
        self.plan.close()


CASES = cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_made_cases(gpu, case):
    """StateWrite -> lsnFusionTemporal -> StateRead on every hand-made sequence."""
    b = Batch([(case.state.size, 1)], case.maps.shape[0])
    b.plan.set_temporal(*case.params)
    b.check(case.maps, case.state, case.params, case.name)
    b.close()


RIGS = {
    "wide_9_ticks": ([(8, 1), (128, 16), (136, 17)], 9, 0),         # the 16-byte form: one chunk, one tile, tiles that end inside
    "odd_5_ticks": ([(1, 1), (7, 15), (9, 17)], 5, 0),              # the element-wise form: below a chunk, odd widths
    "odd_2_ticks": ([(127, 16), (129, 15)], 2, 0),                  # ... one short of a tile and one over
    "one_sensor_1_tick": ([(136, 15)], 1, 0),
    "shifted_5_ticks": ([(128, 17), (8, 16)], 5, 2),                # widths of the 16-byte form, pointers 2 bytes off: element-wise
}


@pytest.mark.parametrize("name", list(RIGS))
def test_frames_across_every_tile_and_chunk_edge(gpu, name):
    """Mixed sensor sizes in one rig, 1 to 3 sensors, n_ticks of 1, 2, 5 and 9; three calls in a row, the history carried from one to the
    next: from none, continued, and continued in place with another setting (which keeps the history)."""
    sizes, T, shift = RIGS[name]
    b = Batch(sizes, T, shift)
    rng = np.random.default_rng(sum(map(ord, name)))
    b.plan.set_temporal(*SETTING)
    b.check(cases.fuzz_maps(rng, b.px, T), None, SETTING, (name, "from no history"))
    taken = np.zeros(6, np.int64)
    maps = cases.fuzz_maps(rng, b.px, T)
    taken += np.bincount(ref.run(maps, b.plan.temporal_state(), *SETTING)[2].ravel(), minlength=6)
    b.check(maps, None, SETTING, (name, "continued"))
    if T >= 2 and b.px * T > 2000:                                  # (one tick behind one tick cannot expire at persist = 2)
        assert (taken[[ref.BLEND, ref.RESTART, ref.FILL, ref.EXPIRE]] > 0).all(), taken     # not vacuous
    other = (255, 4095, 0)
    b.plan.set_temporal(*other)
    b.check(cases.fuzz_maps(rng, b.px, T), None, other, (name, "in place, another setting"), in_place=True)
    b.close()


def test_one_call_equals_split_calls(gpu):
    """The same 5-tick sequence as one call, as 2 + 3, and as five one-tick calls: maps and state identical across the three forms (and
    the restatement's)."""
    sizes = [(136, 17), (9, 5)]
    rng = np.random.default_rng(77)
    px = sum(w * h for w, h in sizes)
    maps = cases.fuzz_maps(rng, px, 5)
    want, wstate, _ = ref.run(maps, np.zeros(px, np.uint32), *SETTING)
    results = []
    for split in ([5], [2, 3], [1, 1, 1, 1, 1]):
        state, outs, t0 = np.zeros(px, np.uint32), [], 0
        plans = {}
        for n in split:
            b = plans.get(n)
            if b is None:
                b = plans[n] = Batch(sizes, n)
                b.plan.set_temporal(*SETTING)
                b.plan.set_temporal_state(state)           # a new plan takes the history over; a plan called again has it
            b.load(maps[t0:t0 + n])
            outs.append(b.run().copy())
            state = b.plan.temporal_state()
            t0 += n
        results.append((np.concatenate(outs), state))
        for b in plans.values():
            b.close()
    for out, state in results:
        assert np.array_equal(out, want) and np.array_equal(state, wstate)


def test_in_place_equals_out_of_place(gpu):
    sizes = [(128, 16), (7, 3)]
    rng = np.random.default_rng(5)
    a, b = Batch(sizes, 5), Batch(sizes, 5)
    maps = cases.fuzz_maps(rng, a.px, 5)
    for x in (a, b):
        x.plan.set_temporal(*SETTING)
        x.load(maps)
    out, inp = a.run().copy(), b.run(in_place=True).copy()
    assert np.array_equal(out, inp) and np.array_equal(a.plan.temporal_state(), b.plan.temporal_state())
    assert np.array_equal(out, ref.run(maps, np.zeros(a.px, np.uint32), *SETTING)[0])
    a.close()
    b.close()


def test_off_copies_refusals_change_nothing_and_reset(gpu):
    import torch
    b = Batch([(136, 17), (7, 5)], 2)
    plan, L = b.plan, native.lib()
    rng = np.random.default_rng(3)
    maps = cases.fuzz_maps(rng, b.px, 2)
    b.load(maps)
    with pytest.raises(native.NativeUtilsError):
        plan.temporal_diagnostics(0)                                # nothing has run yet
    assert not plan.temporal_state().any()
    # off by default: the call copies (in place: nothing) and leaves the history alone
    assert np.array_equal(b.run(), maps) and np.array_equal(b.run(in_place=True), maps)
    assert not plan.temporal_state().any() and not plan.temporal_diagnostics(1).any()
    seeded = ref.run(maps, np.zeros(b.px, np.uint32), 128, 20, 2)[1]
    plan.set_temporal_state(seeded)
    assert np.array_equal(b.run(), maps) and np.array_equal(plan.temporal_state(), seeded)
    # on; every refused setting leaves the previous one in force
    plan.set_temporal(*SETTING)
    state = b.check(maps, seeded, SETTING, "on")
    for bad in [(257, 20, 2), (64, 0, 2), (64, 4096, 2), (64, -1, 2), (64, 20, -1), (64, 20, 256)]:
        assert L.lsnFusionSetTemporal(plan._h, *bad) == -1 and "lsnFusionSetTemporal" in native.last_error(), bad
        state = b.check(maps, None, SETTING, ("after the refused setting", bad))
    # an output that partly overlaps the input is refused with nothing written: maps and history stay; so is a null argument
    b.load(maps)
    before = b.src.buf.cpu().numpy().tobytes()
    for out in (b.src_ptr + 16, b.src_ptr + b.nbytes - 2, b.src_ptr - 2):
        with pytest.raises(native.NativeUtilsError, match="overlap"):
            plan.temporal(b.src_ptr, out)
    b.dst.body().fill_(0x5A)
    assert L.lsnFusionTemporal(plan._h, None, b.dst_ptr, None) == -1 and L.lsnFusionTemporal(plan._h, b.src_ptr, None, None) == -1
    torch.cuda.synchronize()
    assert b.src.buf.cpu().numpy().tobytes() == before and bool((b.dst.body() == 0x5A).all().item())
    assert np.array_equal(plan.temporal_state(), state)
    # StateWrite refuses malformed words and keeps the history
    for word in (1, 255, 65535 * 256 + 1, 0xFFFFFF, 1 << 24, 255 << 24):
        bad = state.copy()
        bad[b.px // 2] = word
        with pytest.raises(native.NativeUtilsError, match="lsnFusionTemporalStateWrite"):
            plan.set_temporal_state(bad)
        assert np.array_equal(plan.temporal_state(), state), word
    for word in (0, 256, 65535 * 256, 256 | (255 << 24)):
        ok = state.copy()
        ok[0] = word
        plan.set_temporal_state(ok)
        assert np.array_equal(plan.temporal_state(), ok)
    # off keeps the history, on again continues it; a reset restarts it
    plan.set_temporal(0)
    assert np.array_equal(b.run(), maps) and np.array_equal(plan.temporal_state(), ok)
    plan.set_temporal(*SETTING)
    b.check(maps, None, SETTING, "on again")
    plan.temporal_reset()
    assert not plan.temporal_state().any()
    b.check(maps, None, SETTING, "after the reset")
    b.close()
