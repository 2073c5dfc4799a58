"""The f64 definition of one ICP step (tests/icp_step_ref.py) and its cases (tests/icp_step_cases.py), tied to the C oracle.

The oracle (oracle/lsn_oracle.c) restates icp.cpp:75-177 line by line with the reference's f32 sequential sums.  Here:
  * every case builder's own conditions hold;
  * the definition and the oracle agree on the match and kept counts of every case exactly, and on Rn within the
    definition's bound (both commit the f32 rounding of M and T that the bound is derived from);
  * apply32 / compose32 reproduce the oracle's moved cloud, R and t BIT FOR BIT from the oracle's own trace, for one
    iteration of every case, from a non-identity start, and for the six-iteration chain.
No GPU involved: this module pins the yardstick that tests/test_icp_step_gpu.py holds the kernels to."""
import numpy as np
import pytest

from tests import icp_step_cases as cases
from tests import icp_step_ref as ref

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_conditions_hold(orc, name):
    c = cases.get(name, orc)
    assert c.step0["m"] >= 1 and len(c.idx) == len(c.src)


def test_winners_follow_the_sequential_scan():
    """The vectorised matching against the loop of icp.cpp:95-126, on clouds of few targets with many exact ties."""
    rng = np.random.default_rng(0)
    for _ in range(20):
        n1, n2 = int(rng.integers(1, 12)), int(rng.integers(1, 200))
        idx = rng.integers(0, n1, size=n2)
        d2 = rng.integers(0, 4, size=n2).astype(F32) * F32(0.25)
        best = {}
        for i in range(n2):
            if idx[i] in best and d2[best[idx[i]]] < d2[i]:
                continue
            best[idx[i]] = i
        assert np.array_equal(ref.winners(idx, d2), np.sort(np.array(list(best.values()))))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_step_against_the_oracles_first_iteration(orc, name):
    c = cases.get(name, orc)
    s = c.step0
    v, R, t, tr = orc.icp(c.tgt, c.src, R=cases.START_R, t=cases.START_T, max_iter=1, nn_mode="brute", trace=True)
    if s["mk"] == 0:
        # the oracle stops before it would reduce an empty matrix: the counts are recorded, nothing moves
        assert (int(tr[0]["n_matched"]), int(tr[0]["n_kept"])) == (s["m"], 0)
        assert not tr[0]["T"].any() and np.array_equal(tr[0]["Rn"].reshape(3, 3), np.eye(3, dtype=F32))
        assert np.array_equal(_bits(v), _bits(c.src)) and np.array_equal(_bits(R), _bits(cases.START_R)) and np.array_equal(_bits(t), _bits(cases.START_T))
        return
    assert (int(tr[0]["n_matched"]), int(tr[0]["n_kept"])) == (s["m"], s["mk"])
    Rn = tr[0]["Rn"].reshape(3, 3)
    if "rank" not in c.waive:
        err = np.abs(Rn.astype(np.float64) - s["Rn"]).max()
        assert err <= ref.bounds(s)["Rn"], (err, ref.bounds(s)["Rn"])
    # the motion and the pose update, from the oracle's own T and Rn
    assert np.array_equal(_bits(ref.apply32(c.src, tr[0]["T"], Rn)), _bits(v))
    R1, t1 = ref.compose32(cases.START_R, cases.START_T, tr[0]["T"], Rn)
    assert np.array_equal(_bits(R1), _bits(R)) and np.array_equal(_bits(t1), _bits(t))


def test_chain_rebuilt_from_the_oracles_trace(orc):
    """Six iterations: the cloud, R and t rebuilt from the trace alone equal the oracle's bit for bit, and every iteration of the
    rebuilt run stays inside the cases' conditions with the definition's counts."""
    c = cases.get("chain", orc)
    v, R, t, tr = orc.icp(c.tgt, c.src, R=cases.START_R, t=cases.START_T, max_iter=6, nn_mode="brute", trace=True)
    cur, Rc, tc = c.src.copy(), cases.START_R, cases.START_T
    for k in range(6):
        idx, d2 = orc.nn(c.tgt, cur, mode="brute", n_threads=8)
        s = ref.step(c.tgt, cur, idx, d2)
        cases.check_conditions(f"chain, iteration {k}", s, c.waive)
        assert (int(tr[k]["n_matched"]), int(tr[k]["n_kept"])) == (s["m"], s["mk"])
        assert np.abs(tr[k]["Rn"].reshape(3, 3) - s["Rn"]).max() <= ref.bounds(s)["Rn"]
        cur = ref.apply32(cur, tr[k]["T"], tr[k]["Rn"])
        Rc, tc = ref.compose32(Rc, tc, tr[k]["T"], tr[k]["Rn"])
    assert np.array_equal(_bits(cur), _bits(v)) and np.array_equal(_bits(Rc), _bits(R)) and np.array_equal(_bits(tc), _bits(t))
    assert np.abs(v - c.src).max() > 1e-3


def test_apply32_rounds_every_operation():
    """apply32 against a per-element evaluation with numpy f32 scalars (one rounding each), and against the double-evaluated and
    the FMA-contracted forms, from each of which it must differ on some element."""
    rng = np.random.default_rng(1)
    v = rng.uniform(-2, 2, size=(4000, 3)).astype(F32)
    T = rng.uniform(-0.1, 0.1, size=3).astype(F32)
    Rn = np.linalg.qr(rng.normal(size=(3, 3)))[0].astype(F32)
    got = ref.apply32(v, T, Rn)
    for i in range(0, 4000, 97):
        x, y, z = F32(v[i, 0] + T[0]), F32(v[i, 1] + T[1]), F32(v[i, 2] + T[2])
        for c in range(3):
            assert got[i, c] == F32(F32(F32(x * Rn[0, c]) + F32(y * Rn[1, c])) + F32(z * Rn[2, c]))
    in_double = ((v.astype(np.float64) + T) @ Rn.astype(np.float64)).astype(F32)
    assert (got != in_double).any()
    # contracted: fma(z, r6, fma(y, r3, x r0)) -- a product of two f32 is exact in f64, so the f64 sum rounded to f32 is the fused result
    # (up to a rare double rounding, which does not matter for "differs somewhere")
    x, y, z = [(v[:, k] + T[k]).astype(np.float64) for k in range(3)]
    R64 = Rn.astype(np.float64)
    fused = np.empty_like(got)
    for c in range(3):
        inner = (y * R64[1, c] + (x * R64[0, c]).astype(F32).astype(np.float64)).astype(F32)
        fused[:, c] = (z * R64[2, c] + inner.astype(np.float64)).astype(F32)
    assert (got != fused).any() and np.abs(got - fused).max() < 1e-5
