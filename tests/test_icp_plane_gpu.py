"""The point-to-plane ICP iteration (lsnIcpRunPlane), held per step to the f64 definition in tests/icp_plane_ref.py.

As tests/test_icp_step_gpu.py does for the point-to-point step: for a run of K iterations, iteration k's input cloud is rebuilt from
the run's own trace with apply32, starting from the source.  Then
  * the run's final cloud equals that rebuild BIT FOR BIT, and the final R, t equal compose32 folded over the trace BIT FOR BIT, from an
    identity and from a non-identity start;
  * every iteration's trace is held to `step` on the rebuilt input: m and mk (the usable count) exact, mean / stddev within
    icp_step_ref.bounds, T / Rn within icp_plane_ref.bounds (both derived from the definitions' own quantities);
  * a step without a usable match, or with g = 0, moves nothing: T = 0 and Rn = I exactly.
Every case runs with the brute-force and the voxel-grid NN; the chain also with the near path off and forced.  The same run twice gives
the same bits; the front half of the step (m, mean, stddev) has lsnIcpRun's bits on every case; and on the corner three plane iterations
end at least a hundred times nearer the walls than ten point-to-point ones.
Each check prints error / bound per quantity (-s shows them); the largest ones measured are recorded in DESIGN.md section 18."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import icp_plane_cases as cases
from tests import icp_plane_ref as pref
from tests import icp_step_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
MODES = [pytest.param(native.NN_BRUTE, id="brute"), pytest.param(native.NN_GRID, id="grid")]
IDENTITY = (np.eye(3, dtype=F32), np.zeros(3, F32))
START = (cases.START_R, cases.START_T)


_bits, _run = cases.bits, cases.run_device


def _check_run(orc, c, out, iters, start, label):
    v, R, t, tr = out
    cur, Rc, tc = np.array(c.src, F32), np.asarray(start[0], F32), np.asarray(start[1], F32)
    for k in range(iters):
        name = f"{label}, iteration {k}"
        if k == 0:
            s = c.step0
        else:
            idx, d2 = orc.nn(c.tgt, cur, mode="brute", n_threads=8)
            s = pref.step(c.tgt, c.nrm, cur, idx, d2)
            cases.check_conditions(name, s, c.waive)
        front = ref.bounds(dict(s, T=np.zeros(3), coord_max=0.0, mk=0))     # mean and sd: the point-to-point step's bounds, as they stand
        b = pref.bounds(s)
        g = tr[k].astype(np.float64)
        gT, gRn = tr[k, 4:7], tr[k, 7:16].reshape(3, 3)
        assert (int(tr[k, 0]), int(tr[k, 1])) == (s["m"], s["mk"]), (name, tr[k, :2], s["m"], s["mk"])
        e_mean = abs(g[2] - s["mean"])
        ratios = {"mean": e_mean / front["mean"]}
        assert e_mean <= front["mean"], (name, "mean", e_mean, front["mean"])
        if "sd" not in c.waive:
            e_sd = abs(g[3] - s["sd"])
            ratios["stddev"] = e_sd / front["sd"]
            assert e_sd <= front["sd"], (name, "stddev", e_sd, front["sd"])
        elif s["dev2"] == 0:
            assert g[3] == 0.0, name
        else:
            # all distances equal up to rounding: only sd's size can be demanded (see tests/test_icp_step_gpu.py)
            cap = np.sqrt(s["sd"] ** 2 + (0.5 * front["mean"]) ** 2 + 8 * ref.EPS64 * s["sum_d2"] / s["m"]) * (1 + 1e-6)
            assert np.isfinite(g[3]) and 0.0 <= g[3] <= cap, (name, "stddev", g[3], cap)
        if s["mk"] == 0 or not s["x"].any():
            assert not gT.any() and np.array_equal(gRn, np.eye(3, dtype=F32)), name
        else:
            e_T, e_Rn = np.abs(g[4:7] - s["T"]), np.abs(gRn.astype(np.float64) - s["Rn"])
            ratios["T"], ratios["Rn"] = float((e_T / b["T"]).max()), float((e_Rn / b["Rn"]).max())
            assert (e_T <= b["T"]).all(), (name, "T", e_T, b["T"])
            assert (e_Rn <= b["Rn"]).all(), (name, "Rn", e_Rn, b["Rn"])
        print(f"ratio {name}: " + " ".join(f"{q}={r:.3f}" for q, r in ratios.items()))
        if s["mk"] > 0:                                   # apply_kernel moves the cloud whenever a match was usable
            cur = ref.apply32(cur, gT, gRn)
            Rc, tc = ref.compose32(Rc, tc, gT, gRn)
    assert np.array_equal(_bits(v), _bits(cur)), f"{label}: the moved cloud is not (v + T) Rn in f32, one rounding per operation"
    assert np.array_equal(_bits(R), _bits(Rc)), f"{label}: R is not R Rn folded over the trace"
    assert np.array_equal(_bits(t), _bits(tc)), f"{label}: t is not t + T R^T (R before its update) folded over the trace"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(cases.CASES))
def test_plane_step_held_to_the_definition(gpu, orc, name, mode):
    c = cases.get(name, orc)
    out = _run(c, c.iters, mode, IDENTITY)
    _check_run(orc, c, out, c.iters, IDENTITY, name)
    if name in cases.NO_MOTION:
        assert np.array_equal(_bits(out[0]), _bits(c.src)) and np.array_equal(out[1], np.eye(3, dtype=F32)) and not out[2].any()
    # the front half is shared: the point-to-point run's m, mean and stddev of iteration 0 have the same bits
    point = _run(c, 1, mode, IDENTITY, plane=False)
    assert np.array_equal(_bits(point[3][0, [0, 2, 3]]), _bits(out[3][0, [0, 2, 3]])), (name, point[3][0, :4], out[3][0, :4])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["chain", "corner", "single_wall", "all_rejected"])
def test_plane_step_from_a_non_identity_start(gpu, orc, name, mode):
    """t += T R^T takes the R of BEFORE the update: from the identity the first iteration cannot tell."""
    c = cases.get(name, orc)
    out = _run(c, c.iters, mode, START)
    _check_run(orc, c, out, c.iters, START, f"{name} from a start pose")
    if name in cases.NO_MOTION:
        assert np.array_equal(_bits(out[0]), _bits(c.src)) and np.array_equal(_bits(out[1]), _bits(cases.START_R)) and np.array_equal(_bits(out[2]), _bits(cases.START_T))


@pytest.mark.parametrize("near", ["0", "2"])
def test_plane_chain_with_the_near_path_off_and_forced(gpu, orc, monkeypatch, near):
    """The seeded NN launch carries the previous iteration's motion: with the near path off and forced, the same definition."""
    monkeypatch.setenv("LSN_ICP_NEAR", near)
    c = cases.get("chain", orc)
    out = _run(c, c.iters, native.NN_GRID, START)
    _check_run(orc, c, out, c.iters, START, f"chain, LSN_ICP_NEAR={near}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["chain", "grid_stride", "single_wall"])
def test_the_same_run_twice_gives_the_same_bits(gpu, orc, name, mode):
    c = cases.get(name, orc)
    a, b = _run(c, c.iters, mode, START), _run(c, c.iters, mode, START)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y)), name


@pytest.mark.parametrize("mode", MODES)
def test_corner_three_plane_iterations_beat_ten_point_to_point(gpu, orc, mode):
    c = cases.get("corner", orc)
    plane = _run(c, 3, mode, IDENTITY)[0]
    point = _run(c, 10, mode, IDENTITY, plane=False)[0]
    start = cases._wall_distance(c.src, c.extra["wall"])
    d_plane, d_point = cases._wall_distance(plane, c.extra["wall"]), cases._wall_distance(point, c.extra["wall"])
    print(f"corner: mean wall distance {start:.3e} m -> {d_plane:.3e} m (lsnIcpRunPlane, 3 iterations), {d_point:.3e} m (lsnIcpRun, 10 iterations)")
    assert 100 * d_plane <= d_point < start, (start, d_plane, d_point)


def test_null_normals_are_an_error(gpu, orc):
    import torch
    c = cases.get("block_edges_63", orc)
    v1, v2 = torch.from_numpy(np.array(c.tgt)).cuda(), torch.from_numpy(np.array(c.src)).cuda()
    Rt = torch.from_numpy(np.concatenate([np.eye(3, dtype=F32).ravel(), np.zeros(3, F32)])).cuda()
    ws = native.IcpWorkspace(0, len(c.tgt), len(c.src))
    try:
        with pytest.raises(native.NativeUtilsError, match="lsnIcpRunPlane"):
            ws.run_plane(v1.data_ptr(), None, len(c.tgt), v2.data_ptr(), len(c.src), Rt.data_ptr(), Rt.data_ptr() + 36, 1, native.NN_GRID, 0)
        torch.cuda.synchronize()
        assert np.array_equal(v2.cpu().numpy(), c.src)
    finally:
        ws.close()
