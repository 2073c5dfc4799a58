"""Seeded clouds with target normals that drive each path of the point-to-plane ICP step (see tests/icp_plane_ref.py).

Every builder returns (tgt, nrm, src[, extra]).  `get(name, orc)` builds a case once, runs the oracle's exact brute-force NN and the
f64 step on it, asserts the regime the exact and bounded demands are fair in, and asserts what the case is named for (`_check_case`),
so that a case that drifts fails loudly instead of weakening a test.  The regime, unless a case waives a part:

  margin   as icp_step_cases.check_conditions: no match within 1e-4 (relative) of the rejection threshold, so the kept count -- and
           with it the usable count -- can be demanded exactly;
  sd       sd >= 1e-3 mean (the one-pass variance keeps its digits);
  modes    every eigenvalue of A is either below 2^-40 lambda_max or above 2^-10 lambda_max: no arithmetic can disagree with the
           definition about the 2^-20 cutoff, and the kept and dropped subspaces are 2^-10 lambda_max apart.
"""
import numpy as np

from tests import icp_plane_ref as pref
from tests import icp_step_cases as pcases
from tests.icp_step_cases import _rot

F32 = np.float32
MARGIN_MIN = pcases.MARGIN_MIN
DROP_BELOW, KEEP_ABOVE = 2.0 ** -40, 2.0 ** -10

CORNER_O = np.array([-1.0, -1.0, -1.0])
TILT = _rot([1, 2, 3], 0.5)


# ---- builders ------------------------------------------------------------------------------------------------------

INSET = 0.25


def _wall_points(rng, n, walls, frame=np.eye(3), size=2.0):
    """n points spread over the given walls of the corner at CORNER_O (wall w is the plane through it with normal e_w, turned by
    `frame` about the corner; a wall starts INSET from the corner's edges, so that a query near an edge has no target of the wrong wall
    next to it).  Returns (points f64, unit normals f64, wall of every point)."""
    w = np.asarray(walls)[rng.integers(0, len(walls), size=n)]
    p = rng.uniform(INSET, size, size=(n, 3))
    p[np.arange(n), w] = 0.0
    e = np.eye(3)[w]
    return CORNER_O + p @ frame.T, e @ frame.T, w


def _wall_distance(pts, wall, frame=np.eye(3)):
    """Mean distance of the points to the wall each was sampled from."""
    e = np.eye(3)[wall] @ frame.T
    return float(np.abs(((np.asarray(pts, np.float64) - CORNER_O) * e).sum(1)).mean())


def _displace(src, angle, shift, axis=(1, -2, 1.5)):
    c = src.mean(axis=0)
    return (src - c) @ _rot(axis, angle).T + c + np.asarray(shift)


def walls(seed, which=(0, 1, 2), frame=None, n1=6000, n2=3000, angle=np.deg2rad(4.0), shift=(0.03, -0.02, 0.02), offset=(0, 0, 0), scale=(1, 1, 1),
          size=2.0, centre_at=None):
    """n1 targets and n2 other samples of the same walls, the samples turned by `angle` about their centre and shifted.  scale: the
    length the normals of wall 0, 1, 2 are given; offset: what the whole scene is shifted by; centre_at: where that shift puts the
    targets' centroid (instead of `offset`)."""
    rng = np.random.default_rng(seed)
    frame = np.eye(3) if frame is None else frame
    tgt, nrm, tw = _wall_points(rng, n1, which, frame, size)
    src, _, sw = _wall_points(rng, n2, which, frame, size)
    src = _displace(src, angle, shift)
    nrm = nrm * np.asarray(scale, np.float64)[tw][:, None]
    off = np.asarray(offset, np.float64) if centre_at is None else np.asarray(centre_at, np.float64) - tgt.mean(axis=0)
    return (tgt + off).astype(F32), nrm.astype(F32), (src + off).astype(F32), dict(wall=sw, frame=frame, offset=off)


def identical(seed):
    tgt, nrm, _, extra = walls(seed, n1=900, n2=10)
    return tgt, nrm, tgt.copy(), extra


def all_rejected(seed):
    """icp_step_cases.pure_translation: every distance equal up to rounding, every match rejected -- whatever the normals say."""
    tgt, src = pcases.pure_translation(seed)
    nrm = np.tile(np.array([0, 0, 1], F32), (len(tgt), 1))
    return tgt, nrm, src, {}


def zero_normals(seed):
    """The corner with a third of the target normals (0, 0, 0) -- what lsnFusionNormals writes for a vertex of no used triangle --, one NaN
    and one Inf: those matches are kept by the rejection and drop out of the sums."""
    tgt, nrm, src, extra = walls(seed, angle=np.deg2rad(1.0), shift=(0.01, -0.01, 0.005))
    nrm = nrm.copy()
    rng = np.random.default_rng(seed + 1000)
    nrm[rng.random(len(nrm)) < 1 / 3] = 0.0
    # the NaN and the Inf go to the targets of the two closest pairs of the scene: matches that win their target and survive the rejection
    d = ((src[:, None, :].astype(np.float64) - tgt[None, :, :].astype(np.float64)) ** 2).sum(-1)
    near = d.argmin(axis=1)
    q = np.argsort(d[np.arange(len(src)), near])
    nan_t = near[q[0]]
    inf_t = near[q[np.flatnonzero(near[q] != nan_t)[0]]]
    nrm[nan_t], nrm[inf_t] = [0.0, np.nan, 1.0], [0.0, 0.0, np.inf]
    extra.update(nan_t=int(nan_t), inf_t=int(inf_t))
    return tgt, nrm, src, extra


def _random_unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def block_edges(n2, seed):
    """icp_step_cases.block_edges (the same clouds, hence the same matching and margins) with random unit normals."""
    tgt, src = pcases.block_edges(n2, seed)
    return tgt, _random_unit(np.random.default_rng(seed + 7), len(tgt)), src, {}


def grid_stride(seed):
    """icp_step_cases.grid_stride: 262 144 + 257 queries, the only shape at which the accumulation loop iterates twice."""
    tgt, src = pcases.grid_stride(seed)
    return tgt, _random_unit(np.random.default_rng(seed + 7), len(tgt)), src, {}


CHAIN_AXES = np.array([0.6, 1.0, 1.7])


def chain(seed):
    """icp_step_cases.chain with analytic normals: the unit gradient of (x / 0.6)^2 + y^2 + (z / 1.7)^2 at every target."""
    tgt, src = pcases.chain(seed)
    g = tgt.astype(np.float64) / CHAIN_AXES ** 2
    g[np.linalg.norm(g, axis=1) == 0] = [0, 0, 1]
    return tgt, (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32), src, {}


# ---- registry ------------------------------------------------------------------------------------------------------
# name -> (builder, arguments, keyword arguments, waived conditions, iterations a run of the case takes)

BLOCK_EDGE_N2 = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
SMALL = dict(angle=np.deg2rad(1.0), shift=(0.01, -0.01, 0.005))

CASES = {
    "corner": (walls, (1,), {}, set(), 3),
    "single_wall": (walls, (2,), dict(which=(2,), frame=TILT, n1=2500, n2=1200, **SMALL), set(), 2),
    "two_walls": (walls, (3,), dict(which=(0, 1), frame=TILT, n1=3000, n2=1500, **SMALL), set(), 2),
    "identical": (identical, (4,), {}, {"sd"}, 1),
    "all_rejected": (all_rejected, (6,), {}, {"sd"}, 2),
    "zero_normals": (zero_normals, (5,), {}, set(), 1),
    "unnormalised": (walls, (13,), dict(scale=(0.5, 3.0, 1.0)), set(), 1),
    "far_from_origin": (walls, (8,), dict(centre_at=(0.0, 5.0, 0.0), size=4.0), set(), 1),
    "grid_stride": (grid_stride, (35,), {}, set(), 1),
    "chain": (chain, (16,), {}, set(), 6),
}
for _n2 in BLOCK_EDGE_N2:
    CASES[f"block_edges_{_n2}"] = (block_edges, (_n2, 100 + _n2), {}, {"sd"} if _n2 == 1 else set(), 2 if _n2 == 1 else 1)

NO_MOTION = ("all_rejected", "block_edges_1")      # mk = 0: everything rejected
FULL_RANK = ("corner", "zero_normals", "unnormalised", "far_from_origin", "grid_stride", "chain") + tuple(f"block_edges_{n}" for n in BLOCK_EDGE_N2[1:])

START_R, START_T = pcases.START_R, pcases.START_T


class Case:
    def __init__(self, name, tgt, nrm, src, idx, d2, step0, waive, iters, extra):
        self.name, self.tgt, self.nrm, self.src, self.idx, self.d2, self.step0 = name, tgt, nrm, src, idx, d2, step0
        self.waive, self.iters, self.extra = waive, iters, extra


def check_conditions(name, s, waive):
    """The regime every (iteration of a) case must be in for the exact and bounded demands to be fair."""
    assert s["margin"] >= MARGIN_MIN, f"{name}: a match lies within {s['margin']:.2e} of the rejection threshold"
    if "sd" not in waive:
        assert s["sd"] >= 1e-3 * s["mean"], f"{name}: sd {s['sd']:.3e} < 1e-3 mean {s['mean']:.3e}"
    if s["mk"] > 0:
        lam = s["lam"]
        ratio = lam / lam.max()
        assert lam.max() > 0 and np.all((ratio < DROP_BELOW) | (ratio > KEEP_ABOVE)), f"{name}: eigenvalue ratios {ratio}"
        assert np.array_equal(s["kept_modes"], ratio > KEEP_ABOVE), name


def killed(s, wrong):
    """How far a wrong variant's motion lies from the definition's, in units of the tolerance `bounds` grants an implementation."""
    b = pref.bounds(s)
    return float(max((np.abs(wrong["T"] - s["T"]) / b["T"]).max(), (np.abs(wrong["Rn"] - s["Rn"]) / b["Rn"]).max()))


def run_chain(orc, tgt, nrm, src, iters, plane=True):
    """The defined chain: exact NN, the f64 step, the motion rounded to f32 and applied with apply32.  Returns (the final cloud, the
    steps).  plane=False: the point-to-point step of icp_step_ref, for comparison."""
    from tests import icp_step_ref as ref
    cur, steps = np.array(src, F32), []
    for _ in range(iters):
        idx, d2 = orc.nn(tgt, cur, mode="brute", n_threads=8)
        s = pref.step(tgt, nrm, cur, idx, d2) if plane else ref.step(tgt, cur, idx, d2)
        steps.append(s)
        if s["mk"] > 0:
            cur = pref.apply32(cur, s["T"].astype(F32), s["Rn"].astype(F32))
    return cur, steps


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def run_device(c, iters, mode, start, plane=True):
    """lsnIcpRunPlane (plane=False: lsnIcpRun) on device arrays of case c, from the pose start = (R, t).  Returns (moved cloud, R, t, trace).
    For the GPU tests."""
    import torch
    from livescan3d_amd import native
    v1 = torch.from_numpy(np.array(c.tgt, F32)).cuda()
    n1 = torch.from_numpy(np.array(c.nrm, F32)).cuda()
    v2 = torch.from_numpy(np.array(c.src, F32)).cuda()
    Rt = torch.from_numpy(np.concatenate([np.asarray(start[0], F32).ravel(), np.asarray(start[1], F32).ravel()])).cuda()
    st = int(torch.cuda.current_stream().cuda_stream)
    ws = native.IcpWorkspace(0, len(c.tgt), len(c.src))
    try:
        if plane:
            ws.run_plane(v1.data_ptr(), n1.data_ptr(), len(c.tgt), v2.data_ptr(), len(c.src), Rt.data_ptr(), Rt.data_ptr() + 36, iters, mode, st)
        else:
            ws.run(v1.data_ptr(), len(c.tgt), v2.data_ptr(), len(c.src), Rt.data_ptr(), Rt.data_ptr() + 36, iters, mode, st)
        tr = ws.trace(iters, st)
        torch.cuda.synchronize()
        v, rt = v2.cpu().numpy(), Rt.cpu().numpy()
    finally:
        ws.close()
    assert len(tr) == iters
    return v, rt[:9].reshape(3, 3), rt[9:], tr


_BUILT = {}


def get(name, orc):
    """The case, its exact NN and its f64 step -- built once, shared by every test, never modified."""
    if name in _BUILT:
        return _BUILT[name]
    builder, args, kwargs, waive, iters = CASES[name]
    tgt, nrm, src, extra = builder(*args, **kwargs)
    tgt, nrm, src = (np.ascontiguousarray(a, F32) for a in (tgt, nrm, src))
    assert max(np.abs(tgt).max(), np.abs(src).max()) < 8.0
    idx, d2 = orc.nn(tgt, src, mode="brute", n_threads=8)
    s = pref.step(tgt, nrm, src, idx, d2)
    check_conditions(name, s, waive)
    c = Case(name, tgt, nrm, src, idx, d2, s, waive, iters, extra)
    _check_case(c, orc)
    for a in (tgt, nrm, src, idx, d2):
        a.setflags(write=False)
    _BUILT[name] = c
    return c


def _check_case(c, orc):
    """What each case is there for."""
    name, s = c.name, c.step0
    lam, kept = s["lam"], s["kept_modes"]
    if name in NO_MOTION:
        assert s["mk"] == 0 and s["n_kept"] == 0 and not s["T"].any() and np.array_equal(s["Rn"], np.eye(3))
    else:
        assert s["mk"] > 0
    if name in FULL_RANK:
        assert kept.all(), (name, lam / lam.max())
    if name == "corner":
        wall = c.extra["wall"]
        start = _wall_distance(c.src, wall)
        plane, _ = run_chain(orc, c.tgt, c.nrm, c.src, 3)
        point, _ = run_chain(orc, c.tgt, c.nrm, c.src, 10, plane=False)
        d_plane, d_point = _wall_distance(plane, wall), _wall_distance(point, wall)
        c.extra["chain_distances"] = (start, d_plane, d_point)
        assert len(c.tgt) == 6000 and len(c.src) == 3000 and start > 0.03
        assert 100 * d_plane <= d_point, (start, d_plane, d_point)
    if name in ("single_wall", "two_walls"):
        n_drop = 3 if name == "single_wall" else 1
        assert (~kept).sum() == n_drop, lam / lam.max()
        assert np.abs(s["V"][:, ~kept].T @ s["x"]).max() <= 1e-14 * np.linalg.norm(s["x"]) and np.linalg.norm(s["x"]) > 1e-3
        e = np.eye(3) @ c.extra["frame"].T                     # the zero modes the geometry predicts lie in the dropped subspace
        if name == "single_wall":
            n = e[2]
            u = np.cross(n, [1, 0, 0]); u /= np.linalg.norm(u)
            modes = [np.concatenate([np.zeros(3), u]), np.concatenate([np.zeros(3), np.cross(n, u)]), np.concatenate([n, np.zeros(3)])]
        else:
            modes = [np.concatenate([np.zeros(3), np.cross(e[0], e[1])])]
        Vk = s["V"][:, kept]
        for z in modes:
            assert np.linalg.norm(Vk.T @ z) <= 1e-6 * np.linalg.norm(z), (name, Vk.T @ z)
    if name == "identical":
        assert s["mk"] == s["m"] == len(c.src) and not c.d2.any() and not s["g"].any() and not s["x"].any()
        assert not s["T"].any() and np.array_equal(s["Rn"], np.eye(3))
    if name == "all_rejected":
        assert s["m"] == len(c.tgt)
    if name == "zero_normals":
        tk = c.idx[s["winners"][s["keep"]]]                     # the kept matches' targets
        assert c.extra["nan_t"] in tk and c.extra["inf_t"] in tk and np.isnan(c.nrm[c.extra["nan_t"]]).any() and np.isinf(c.nrm[c.extra["inf_t"]]).any()
        with np.errstate(invalid="ignore"):
            zero = ~np.asarray(c.nrm[tk]).any(axis=1)
        assert s["mk"] == s["n_kept"] - zero.sum() - 2 and 0.25 * s["n_kept"] < zero.sum() < 0.42 * s["n_kept"] and s["kept_modes"].all()
        # the step on the cloud with those matches removed, stated independently: least squares over the rows of the remaining matches
        wk = s["winners"][s["keep"]]
        good = np.isfinite(c.nrm[tk]).all(axis=1) & ~zero
        J, r = pref.terms(c.tgt[tk[good]], c.nrm[tk[good]], c.src[wk[good]])
        x = np.linalg.lstsq(J, -r, rcond=None)[0]
        assert len(r) == s["mk"] and np.abs(x - s["x"]).max() <= 1e-12 * np.abs(x).max()
    if name == "unnormalised":
        ln = np.linalg.norm(c.nrm.astype(np.float64), axis=1)
        assert {0.5, 3.0, 1.0} == set(np.round(ln, 6).tolist())
        unit = pref.step(c.tgt, (c.nrm / ln[:, None]).astype(F32), c.src, c.idx, c.d2)
        assert unit["mk"] == s["mk"] and killed(s, unit) > 100
    if name == "far_from_origin":
        A = s["A"]
        coupling = np.linalg.norm(A[:3, 3:], 2) / np.sqrt(np.linalg.norm(A[:3, :3], 2) * np.linalg.norm(A[3:, 3:], 2))
        assert np.linalg.norm(c.tgt.astype(np.float64).mean(axis=0)) >= 5.0 - 1e-6 and coupling > 0.9, coupling
    if name.startswith("block_edges") and name not in NO_MOTION:
        assert len(c.src) == int(name.split("_")[-1])
    if name in ("block_edges_1023", "block_edges_1024", "block_edges_1025"):
        assert not np.any((s["winners"] >= 256) & (s["winners"] < 512)), "the second workgroup has a winner"
    if name == "grid_stride":
        assert len(c.src) == 262144 + 257 and s["m"] > 1024
    if c.iters > 1:                                        # every iteration of the defined chain stays in the regime and keeps the case's rank
        _, steps = run_chain(orc, c.tgt, c.nrm, c.src, c.iters)
        for k, sk in enumerate(steps):
            check_conditions(f"{name}, iteration {k}", sk, c.waive)
            assert np.array_equal(sk["kept_modes"], kept) and (name != "chain" or sk["mk"] < sk["m"]), (name, k)
