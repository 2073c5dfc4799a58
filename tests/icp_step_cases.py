"""Seeded clouds that drive each path of the ICP step after the neighbour search (see tests/icp_step_ref.py).

Every builder returns (tgt, src).  `get(name, orc)` builds a case once, runs the exact brute-force NN of the oracle and the f64
step on it, and asserts the case's own conditions, so that a case that drifts out of its regime fails loudly instead of
weakening a test.  Unless a case says otherwise (its `waive` set):

  margin   the smallest |d - thresh| / thresh over the matches is >= 1e-4: an f32 threshold differs from the f64 one by
           about 1e-6 relative, so with a hundredfold margin the kept count can be demanded exactly -- with no match left out;
  sd       sd >= 1e-3 mean: the one-pass variance keeps its digits;
  rank     sigma2 + sigma3 >= sigma1 / 50: the polar factor is well determined (M is uncentred in the reference, so clouds far
           from the origin are ill-conditioned there too; coordinates stay within a few metres of the origin).
"""
import numpy as np

from tests import icp_step_ref as ref

F32 = np.float32
MARGIN_MIN = 1e-4


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _jittered_grid(rng, nx, ny, pitch, jitter):
    """nx x ny points in the plane, at least pitch - 2 jitter apart."""
    g = np.stack(np.meshgrid(np.arange(nx) - (nx - 1) / 2, np.arange(ny) - (ny - 1) / 2, indexing="ij"), -1).reshape(-1, 2) * pitch
    return g + rng.uniform(-jitter, jitter, size=g.shape)


# ---- builders ------------------------------------------------------------------------------------------------------

def block_edges(n2, seed):
    """n2 queries around the sizes of a wave, a workgroup and a few workgroups, against 300 targets.  From four workgroups on,
    queries 256..511 are all losers: they crowd around target 0, which query 3 sits closest to.  That is the second workgroup of
    stats_kernel and accum_kernel, which walk the queries by their original index: a block whose partial sums are all zero.  (The
    claim kernels run in cell order; for them this is simply 256 claims on one target.)"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(300, 3))
    src = rng.uniform(-1, 1, size=(n2, 3))
    if n2 >= 1023:
        tgt[0] = [2.5, 2.5, 2.5]
        src[3] = tgt[0] + [0.01, 0, 0]
        d = rng.normal(size=(256, 3))
        src[256:512] = tgt[0] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.05, 0.2, size=(256, 1))
    return tgt.astype(F32), src.astype(F32)


def many_onto_few(seed):
    """3000 queries around 40 targets: every workgroup piles its claims onto a few slots of the LDS claim table."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(40, 3))
    src = tgt[rng.integers(0, 40, size=3000)] + rng.normal(scale=0.05, size=(3000, 3))
    return tgt.astype(F32), src.astype(F32)


COLLIDING = (7, 1031, 2055, 3079, 4103)   # all k & 1023 == 7
N_STRAY = 24


def slot_collisions(seed):
    """5 x 1024 targets of which only five, all with k & 1023 == 7, lie near the queries: one claim-table slot, five
    targets, so four of them take the global path in every workgroup (a few stray queries aside, see below).  The kernels process queries in cell order, so the
    mix must hold spatially: the queries form a thin column along z, the five targets ring it in the plane z = 0 (z adds the
    same z^2 to all five distances), and a query's neighbour is decided by the direction of its small offset from the axis.
    The order inside a cell is the arrival order of the grid build's atomics and cannot be asserted from here; the offset
    directions are independent of index and of z, and `get` asserts the mix for every 200 queries consecutive by index or along z.
    The result does not depend on the order either way."""
    rng = np.random.default_rng(seed)
    n2 = 1500
    far = rng.normal(size=(5 * 1024, 3))
    tgt = far / np.linalg.norm(far, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, size=(len(far), 1))
    for j, k in enumerate(COLLIDING):
        th = 2 * np.pi * j / 5 + 0.3
        r = 0.30 + 0.0005 * j
        tgt[k] = [r * np.cos(th), r * np.sin(th), 0.0]
    th = rng.uniform(0, 2 * np.pi, size=n2)
    eps = rng.uniform(0.005, 0.02, size=n2)
    src = np.stack([eps * np.cos(th), eps * np.sin(th), rng.uniform(-0.5, 0.5, size=n2)], axis=1)
    # the five winners' distances are all about 0.3^2, and d > 2.5 sd would reject every one of them: a few stray queries out
    # among the far targets give the distances a spread (they claim other slots)
    stray = rng.permutation(n2)[:N_STRAY]
    d = rng.normal(size=(N_STRAY, 3))
    src[stray] = tgt[rng.permutation(len(tgt))[:N_STRAY]] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.4, 1.0, size=(N_STRAY, 1))
    return tgt.astype(F32), src.astype(F32)


def exact_ties(seed):
    """Pairs of queries that mirror each other about their shared target with power-of-two offsets: the two f32 distances are
    bit-equal and the LATER query must win.  Several offsets, so that sd > 0 and the smaller pairs survive the rejection; the
    query order is shuffled (the kernels process queries in cell order, not index order), with the +offset partner always at the
    higher index, so the wrong tie rule moves T by twice the mean offset."""
    rng = np.random.default_rng(seed)
    lat = np.stack(np.meshgrid(np.arange(-2, 3), np.arange(-2, 3), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3) * 0.5
    tgt = lat[rng.permutation(len(lat))]
    n = len(tgt)
    k = rng.integers(5, 9, size=n)                       # offsets 2^-5 .. 2^-8
    off = np.zeros((n, 3))
    off[np.arange(n), rng.integers(0, 3, size=n)] = 2.0 ** -k
    extra = rng.integers(0, 3, size=n)                   # a second component on some pairs: more distinct distances
    add = (rng.random(n) < 0.5) & (off[np.arange(n), extra] == 0)
    off[np.arange(n)[add], extra[add]] = 2.0 ** -(k[add] + 1)
    plus, minus = tgt + off, tgt - off
    perm = rng.permutation(2 * n)
    pos_plus, pos_minus = perm[:n].copy(), perm[n:].copy()
    swap = pos_plus < pos_minus
    pos_plus[swap], pos_minus[swap] = pos_minus[swap], pos_plus[swap].copy()
    src = np.zeros((2 * n, 3))
    src[pos_plus], src[pos_minus] = plus, minus
    return tgt.astype(F32), src.astype(F32)


def noise_with_outliers(seed):
    """A noisy copy of part of the target with 2 % far outliers: the rejection has something to reject."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(2000, 3))
    src = tgt[rng.permutation(2000)[:1500]] + rng.normal(scale=0.01, size=(1500, 3))
    out = rng.permutation(1500)[:30]
    src[out] += rng.normal(scale=0.5, size=(30, 3))
    return tgt.astype(F32), src.astype(F32)


def identical(seed):
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(700, 3)).astype(F32)
    return tgt, tgt.copy()


def pure_translation(seed):
    """A cloud and its translation by less than half the point spacing: every distance equal up to rounding, sd ~ 0, all
    matches rejected.  The reference would throw in cv::reduce on the empty matrix; the defined behaviour is no motion."""
    rng = np.random.default_rng(seed)
    xy = _jittered_grid(rng, 20, 20, 0.1, 0.02)
    tgt = np.concatenate([xy, rng.uniform(-0.5, 0.5, size=(len(xy), 1))], axis=1)
    src = tgt.astype(F32).astype(np.float64) + [0.011, -0.007, 0.005]
    return tgt.astype(F32), src.astype(F32)


def one_one(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, size=(1, 3)).astype(F32), rng.uniform(-1, 1, size=(1, 3)).astype(F32)


def _nn_is_identity(tgt, src):
    d = ((src[:, None, :].astype(np.float64) - tgt[None, :, :].astype(np.float64)) ** 2).sum(-1)
    return bool((d.argmin(axis=1) == np.arange(len(src))).all())


def rotation(axis, seed):
    """500 well-spaced points on an ellipsoid about 2 m from the origin, rotated about `axis` by the largest angle (of a
    geometric ladder) that keeps every query's neighbour its own partner."""
    rng = np.random.default_rng(seed)
    i = np.arange(500) + 0.5
    phi = np.arccos(1 - 2 * i / 500)
    th = np.pi * (1 + 5 ** 0.5) * i
    tgt = np.stack([2.0 * np.cos(th) * np.sin(phi), 1.6 * np.sin(th) * np.sin(phi), 1.3 * np.cos(phi)], axis=1)
    tgt = (tgt + rng.normal(scale=0.004, size=tgt.shape)).astype(F32)
    angle = 0.2
    while True:
        src = (tgt.astype(np.float64) @ _rot(axis, angle).T).astype(F32)
        if _nn_is_identity(tgt, src):
            break
        angle *= 0.85
        assert angle > 1e-3
    assert _nn_is_identity(tgt, src)
    return tgt, src


def rank2(seed):
    """A plane through the origin (z = 0 exactly) rotated in its plane: M's third row and column are exactly zero, sigma3 = 0,
    and svd3 completes U by a cross product."""
    rng = np.random.default_rng(seed)
    xy = _jittered_grid(rng, 20, 20, 0.15, 0.03)
    tgt = np.concatenate([xy, np.zeros((len(xy), 1))], axis=1).astype(F32)
    src = (tgt.astype(np.float64) @ _rot([0, 0, 1], 0.02).T).astype(F32)
    assert not src[:, 2].any() and _nn_is_identity(tgt, src)
    return tgt, src


def reflection(seed):
    """A thin slab (+-1 cm, points at least 6 cm apart in the plane) against its mirror image through the mid-plane: the
    pairing is intact, det M < 0, and the determinant fix decides the answer."""
    rng = np.random.default_rng(seed)
    xy = _jittered_grid(rng, 20, 20, 0.1, 0.02)
    tgt = np.concatenate([xy, rng.uniform(-0.01, 0.01, size=(len(xy), 1))], axis=1).astype(F32)
    src = tgt * np.array([1, 1, -1], F32)
    assert _nn_is_identity(tgt, src)
    return tgt, src


def rank1(direction, seed):
    """Collinear points through the origin against a stretched, shifted copy: the reference's rotation is not unique."""
    rng = np.random.default_rng(seed)
    e = np.asarray(direction, np.float64)
    e = e / np.linalg.norm(e)
    s = np.sort(rng.uniform(-1.5, 1.5, size=300))
    s = s[np.concatenate([[True], np.diff(s) > 0.004])]
    tgt = (s[:, None] * e).astype(F32)
    src = ((s * 1.0005 + 0.0011)[:, None] * e).astype(F32)
    return tgt, src


def grid_stride(seed):
    """262 144 + 257 queries: the only shape at which the grid-stride loops of stats_kernel and accum_kernel iterate
    (1024 workgroups x 256 threads cover 262 144 queries in one trip)."""
    rng = np.random.default_rng(seed)
    n2 = 262144 + 257
    tgt = rng.uniform(-1, 1, size=(2048, 3))
    src = tgt[rng.integers(0, 2048, size=n2)] + rng.normal(scale=0.03, size=(n2, 3))
    return tgt.astype(F32), src.astype(F32)


def chain(seed):
    """4000 targets and 2500 queries: a rotated, shifted, noisy copy with outliers, for a run of six iterations."""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1, 1, size=(4000, 3)) * [1.5, 1.0, 0.7]
    src = tgt[rng.permutation(4000)[:2500]] @ _rot([1, 2, 3], 0.01).T + [0.004, -0.003, 0.002] + rng.normal(scale=0.003, size=(2500, 3))
    out = rng.permutation(2500)[:50]
    src[out] += rng.normal(scale=0.4, size=(50, 3))
    return tgt.astype(F32), src.astype(F32)


# ---- registry ------------------------------------------------------------------------------------------------------
# name -> (builder, arguments, waived conditions, expected (m, mk) where the case states them).  The seeds are ordinary ones;
# where the first seed tried left a match within 1e-4 of the threshold the next one was taken.

BLOCK_EDGE_N2 = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025)

CASES = {}
for _n2 in BLOCK_EDGE_N2:
    # n2 = 1: one match, sd = 0, thresh = 0, and d > 0 is rejected: no motion.  n2 = 2: two matches d1 < d2, sd = (d2 - d1) / 2,
    # thresh = 1.25 (d2 - d1): d1 stays when d1 <= 5/9 d2, d2 only when d2 >= 5 d1.  This seed keeps d1 alone: M = (b + T) a^T has
    # rank 1 and only the rank-1 demands apply to Rn.
    CASES[f"block_edges_{_n2}"] = (block_edges, (_n2, 101 if _n2 == 2 else 100 + _n2), {1: {"sd", "rank"}, 2: {"rank"}}.get(_n2, set()))
CASES["many_onto_few"] = (many_onto_few, (1,), set())
CASES["slot_collisions"] = (slot_collisions, (2,), set())
CASES["exact_ties"] = (exact_ties, (3,), set())
CASES["noise_with_outliers"] = (noise_with_outliers, (4,), set())
CASES["identical"] = (identical, (5,), {"sd"})
CASES["pure_translation"] = (pure_translation, (6,), {"sd", "rank"})
CASES["one_one"] = (one_one, (7,), {"sd", "rank"})
CASES["rotation_x"] = (rotation, ([1, 0, 0], 18), set())
CASES["rotation_y"] = (rotation, ([0, 1, 0], 9), set())
CASES["rotation_diag"] = (rotation, ([1, -2, 3], 10), set())
CASES["rank2"] = (rank2, (11,), set())
CASES["reflection"] = (reflection, (12,), set())
CASES["rank1_axis"] = (rank1, ([1, 0, 0], 13), {"rank"})
CASES["rank1_oblique"] = (rank1, ([1, 2, -3], 14), {"rank"})
CASES["grid_stride"] = (grid_stride, (35,), set())
CASES["chain"] = (chain, (16,), set())

NO_MOTION = ("block_edges_1", "pure_translation", "one_one")   # mk = 0: everything rejected
RANK1 = ("rank1_axis", "rank1_oblique", "block_edges_2")

# a real rotation and a non-zero translation to start from (the pose the caller hands in; the cloud is what it is)
START_R = _rot([2, -1, 1], 0.7).astype(F32)
START_T = np.array([0.25, -1.5, 0.75], F32)


class Case:
    def __init__(self, name, tgt, src, idx, d2, step0, waive):
        self.name, self.tgt, self.src, self.idx, self.d2, self.step0, self.waive = name, tgt, src, idx, d2, step0, waive


def check_conditions(name, s, waive):
    """The regime every (iteration of a) case must be in for the exact and bounded demands to be fair."""
    assert s["margin"] >= MARGIN_MIN, f"{name}: a match lies within {s['margin']:.2e} of the rejection threshold"
    if "sd" not in waive:
        assert s["sd"] >= 1e-3 * s["mean"], f"{name}: sd {s['sd']:.3e} < 1e-3 mean {s['mean']:.3e}"
    if "rank" not in waive:
        sg = s["sigma"]
        assert s["mk"] > 0 and sg[1] + sg[2] >= sg[0] / 50, f"{name}: singular values {sg}"


_BUILT = {}


def get(name, orc):
    """The case, its exact NN and its f64 step -- built once, shared by every test, never modified."""
    if name in _BUILT:
        return _BUILT[name]
    builder, args, waive = CASES[name]
    tgt, src = builder(*args)
    tgt, src = np.ascontiguousarray(tgt, F32), np.ascontiguousarray(src, F32)
    assert max(np.abs(tgt).max(), np.abs(src).max()) < 8.0
    idx, d2 = orc.nn(tgt, src, mode="brute", n_threads=8)
    s = ref.step(tgt, src, idx, d2)
    check_conditions(name, s, waive)
    _check_case(name, tgt, src, idx, d2, s)
    for a in (tgt, src, idx, d2):
        a.setflags(write=False)
    _BUILT[name] = Case(name, tgt, src, idx, d2, s, waive)
    return _BUILT[name]


def _check_case(name, tgt, src, idx, d2, s):
    """What each case is there for."""
    n2 = len(src)
    if name in NO_MOTION:
        assert s["mk"] == 0 and s["m"] == (len(tgt) if name == "pure_translation" else 1)
    else:
        assert s["mk"] > 0
    if name in ("block_edges_1023", "block_edges_1025"):
        assert not np.any((s["winners"] >= 256) & (s["winners"] < 512)), "the second workgroup has a winner"
    if name == "block_edges_2":
        assert s["m"] == 2 and s["mk"] == 1
    if name == "many_onto_few":
        assert s["m"] == 40
    if name == "slot_collisions":
        near = np.isin(idx, COLLIDING)
        assert near.sum() == n2 - N_STRAY and set(idx[near].tolist()) == set(COLLIDING) and 5 < s["m"] <= 5 + N_STRAY
        assert np.isin(idx[s["kept"]], COLLIDING).sum() == 5, "a colliding target's match was rejected"
        for order in (np.arange(n2), np.argsort(src[:, 2], kind="stable")):   # any 200 queries consecutive by index or along z claim all five
            seq = idx[order]
            for a in range(0, n2 - 200, 50):
                assert set(COLLIDING) <= set(seq[a:a + 200].tolist())
    if name == "exact_ties":
        n = len(tgt)
        assert n2 == 2 * n and s["m"] == n and 0 < s["mk"] < n and s["sd"] > 0
        order = np.lexsort((np.arange(n2), idx))
        assert np.array_equal(idx[order][0::2], idx[order][1::2]) and np.array_equal(d2[order][0::2].view(np.uint32), d2[order][1::2].view(np.uint32))
        wrong = ref.step(tgt, src, idx, d2, tie="first")
        assert wrong["mk"] == s["mk"] and not np.intersect1d(wrong["winners"], s["winners"]).size
        assert np.abs(wrong["T"] - s["T"]).max() > 100 * ref.bounds(s)["T"].max()
    if name == "noise_with_outliers":
        assert s["mk"] < s["m"]
    if name == "identical":
        assert s["mk"] == s["m"] == n2 and not d2.any() and not s["T"].any()
    if name.startswith("rotation") or name in ("rank2", "reflection"):
        assert np.array_equal(idx, np.arange(n2)) and s["m"] == n2
    if name == "rank2":
        assert s["sigma"][2] == 0.0
    if name == "reflection":
        M = s["M"]
        U, sg, Vt = np.linalg.svd(M)
        assert np.linalg.det(M) < 0 and np.linalg.det(U @ Vt) < 0 and s["flipped"] and sg[2] <= sg[1] / 4
    if name in RANK1:
        assert s["sigma"][1] <= 1e-5 * s["sigma"][0]
    if name == "grid_stride":
        assert n2 == 262144 + 257 and s["m"] > 1024
