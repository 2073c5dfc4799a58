"""The ICP iteration after the neighbour search, held per step to the f64 definition in tests/icp_step_ref.py.

For a run of K iterations, iteration k's input cloud is rebuilt from the run's own trace with apply32, starting from the
source.  Then:
  * the run's final cloud equals that rebuild BIT FOR BIT (either apply path; no contraction, no other association);
  * the final R, t equal compose32 folded over the trace BIT FOR BIT, from an identity and from a non-identity start;
  * every iteration's trace is held to `step` on the rebuilt input: m and mk exact, mean / stddev / T / Rn within
    `bounds` (derived there from the definition's own quantities);
  * a step that rejects every match moves nothing: cloud, R, t untouched bit for bit, T = 0, Rn = I in the trace;
  * rank-1 inputs, where the reference's rotation is not unique: finite, orthonormal to 1e-6, det = +1, and the mean squared
    distance of the kept pairs does not grow.
Every case runs with the brute-force and the voxel-grid NN; the chain also with the near path off and forced.
Each check prints error / bound per quantity (-s shows them); the largest ones measured are recorded in DESIGN.md."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import icp_step_cases as cases
from tests import icp_step_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = [pytest.param(native.NN_BRUTE, id="brute"), pytest.param(native.NN_GRID, id="grid")]
IDENTITY = (np.eye(3, dtype=F32), np.zeros(3, F32))
START = (cases.START_R, cases.START_T)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _run(tgt, src, iters, mode, start):
    """lsnIcpRun on device arrays.  Returns (moved cloud, R, t, trace)."""
    import torch
    v1 = torch.from_numpy(np.ascontiguousarray(tgt, F32)).cuda()
    v2 = torch.from_numpy(np.array(src, F32)).cuda()
    Rt = torch.from_numpy(np.concatenate([np.asarray(start[0], F32).ravel(), np.asarray(start[1], F32).ravel()])).cuda()
    st = int(torch.cuda.current_stream().cuda_stream)
    ws = native.IcpWorkspace(0, len(tgt), len(src))
    try:
        ws.run(v1.data_ptr(), len(tgt), v2.data_ptr(), len(src), Rt.data_ptr(), Rt.data_ptr() + 36, iters, mode, st)
        tr = ws.trace(iters, st)
        torch.cuda.synchronize()
        v, rt = v2.cpu().numpy(), Rt.cpu().numpy()
    finally:
        ws.close()
    assert len(tr) == iters
    return v, rt[:9].reshape(3, 3), rt[9:], tr


def _check_run(orc, c, out, iters, start, label):
    v, R, t, tr = out
    cur, Rc, tc = np.array(c.src, F32), np.asarray(start[0], F32), np.asarray(start[1], F32)
    for k in range(iters):
        name = f"{label}, iteration {k}"
        if k == 0:
            idx, s = c.idx, c.step0
        else:
            idx, d2 = orc.nn(c.tgt, cur, mode="brute", n_threads=8)
            s = ref.step(c.tgt, cur, idx, d2)
            cases.check_conditions(name, s, c.waive)
        b = ref.bounds(s)
        g = tr[k].astype(np.float64)
        gT, gRn = tr[k, 4:7], tr[k, 7:16].reshape(3, 3)
        assert (int(tr[k, 0]), int(tr[k, 1])) == (s["m"], s["mk"]), name
        e_mean = abs(g[2] - s["mean"])
        ratios = {"mean": e_mean / b["mean"]}
        assert e_mean <= b["mean"], (name, "mean", e_mean, b["mean"])
        if "sd" not in c.waive:
            e_sd = abs(g[3] - s["sd"])
            ratios["stddev"] = e_sd / b["sd"]
            assert e_sd <= b["sd"], (name, "stddev", e_sd, b["sd"])
        elif s["dev2"] == 0:
            assert g[3] == 0.0, name                      # one match, or all distances zero: exactly no spread
        else:
            # all distances equal up to rounding (sd << ulp(mean)): the deviations are taken from the f32 mean, as the reference
            # takes them, so sd's relative error is O(1) and only its size can be demanded: sum (d - mean32)^2 =
            # sum (d - mu)^2 + m (mu - mean32)^2, the second term at most m (ulp / 2)^2, plus the one-pass cancellation
            cap = np.sqrt(s["sd"] ** 2 + (0.5 * b["mean"]) ** 2 + 8 * ref.EPS64 * s["sum_d2"] / s["m"]) * (1 + 1e-6)
            assert np.isfinite(g[3]) and 0.0 <= g[3] <= cap, (name, "stddev", g[3], cap)
        if s["mk"] == 0:
            assert not gT.any() and np.array_equal(gRn, np.eye(3, dtype=F32)), name
            print(f"ratio {name}: " + " ".join(f"{q}={r:.3f}" for q, r in ratios.items()))
            continue
        e_T = np.abs(g[4:7] - s["T"])
        ratios["T"] = float((e_T / b["T"]).max())
        assert (e_T <= b["T"]).all(), (name, "T", e_T, b["T"])
        if "rank" not in c.waive:
            e_Rn = np.abs(gRn.astype(np.float64) - s["Rn"]).max()
            ratios["Rn"] = e_Rn / b["Rn"]
            assert e_Rn <= b["Rn"], (name, "Rn", e_Rn, b["Rn"])
        else:
            Rn64 = gRn.astype(np.float64)
            assert np.isfinite(Rn64).all() and np.abs(Rn64 @ Rn64.T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(Rn64) - 1) <= 1e-6, name
            a = c.tgt[idx[s["kept"]]].astype(np.float64)
            before = ((a - cur[s["kept"]].astype(np.float64)) ** 2).sum(1).mean()
            after = ((a - ref.apply32(cur, gT, gRn)[s["kept"]].astype(np.float64)) ** 2).sum(1).mean()
            assert after <= before, (name, before, after)
        print(f"ratio {name}: " + " ".join(f"{q}={r:.3f}" for q, r in ratios.items()))
        cur = ref.apply32(cur, gT, gRn)
        Rc, tc = ref.compose32(Rc, tc, gT, gRn)
    assert np.array_equal(_bits(v), _bits(cur)), f"{label}: the moved cloud is not (v + T) Rn in f32, one rounding per operation"
    assert np.array_equal(_bits(R), _bits(Rc)), f"{label}: R is not R Rn folded over the trace"
    assert np.array_equal(_bits(t), _bits(tc)), f"{label}: t is not t + T R^T (R before its update) folded over the trace"


def _iters(name):
    return 6 if name == "chain" else (2 if name in cases.NO_MOTION else 1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_step_held_to_the_definition(gpu, orc, name, mode):
    c = cases.get(name, orc)
    out = _run(c.tgt, c.src, _iters(name), mode, IDENTITY)
    _check_run(orc, c, out, _iters(name), IDENTITY, name)
    if name in cases.NO_MOTION:
        assert np.array_equal(_bits(out[0]), _bits(c.src)) and np.array_equal(out[1], np.eye(3, dtype=F32)) and not out[2].any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["chain", "noise_with_outliers", "reflection", "pure_translation"])
def test_step_from_a_non_identity_start(gpu, orc, name, mode):
    """t += T R^T takes the R of BEFORE the update: from the identity the first iteration cannot tell."""
    c = cases.get(name, orc)
    out = _run(c.tgt, c.src, _iters(name), mode, START)
    _check_run(orc, c, out, _iters(name), START, f"{name} from a start pose")
    if name in cases.NO_MOTION:
        assert np.array_equal(_bits(out[0]), _bits(c.src)) and np.array_equal(_bits(out[1]), _bits(cases.START_R)) and np.array_equal(_bits(out[2]), _bits(cases.START_T))


@pytest.mark.parametrize("near", ["0", "2"])
def test_chain_with_the_near_path_off_and_forced(gpu, orc, monkeypatch, near):
    """The seeded NN launch carries the previous iteration's motion: with the near path off and forced, the same definition."""
    monkeypatch.setenv("LSN_ICP_NEAR", near)
    c = cases.get("chain", orc)
    out = _run(c.tgt, c.src, 6, native.NN_GRID, START)
    _check_run(orc, c, out, 6, START, f"chain, LSN_ICP_NEAR={near}")


def test_host_export_returns_the_device_runs_bits(gpu, orc):
    c = cases.get("chain", orc)
    v, R, t, _ = _run(c.tgt, c.src, 6, native.NN_GRID, START)
    hv, hR, ht = native.icp(c.tgt, c.src, R=cases.START_R, t=cases.START_T, max_iter=6)
    assert np.array_equal(_bits(hv), _bits(v)) and np.array_equal(_bits(hR), _bits(R)) and np.array_equal(_bits(ht), _bits(t))
