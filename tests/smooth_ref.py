"""Mesh smoothing (lsnFusionSmooth) restated in numpy: the definition the kernels are held to bit for bit.

The reference smooths nothing; nothing here is pinned to it.  One pass with factor f goes from float32 positions P to P', reading only P.
A triangle is USED iff its indices are in [0, nVertices), pairwise distinct, and the nine coordinates of its corners in P satisfy
|c| < 4096 (in float32; NaN and inf fail).  q(c) = int64(trunc(c * 2^32)), exact.  A used triangle adds, at each corner, the q of its two
other corners to the corner's three int64 sums S (wrap-around) and 2 to its count N.  N == 0 or a pinned vertex: P' = P bit for bit; else
m = float32((float64(S) / float64(N)) * 2^-32), d = m - p, p' = p + f * d, every float32 operation rounded on its own.

Open vertices, from the indices alone: every triangle that is in range and pairwise distinct adds mix(next) - mix(previous) to the uint64
H of each corner (wrap-around), mix the splitmix64 finaliser; a vertex is open iff H != 0.  With pin_boundary they are pinned in every pass.

The filter: `iterations` times a pass with lambda then one with mu (left out when mu == 0).

`mutant` (tests only) names one deliberate departure from the definition; tests/test_smooth_ref.py asserts that the hand-made cases of
tests/smooth_cases.py tell each of them from the definition."""
import numpy as np

LIMIT = np.float32(4096.0)
SCALE = np.float32(2.0 ** 32)
MUTANTS = ("floor", "dedup", "count_one", "no_mu", "gauss_seidel", "no_pin", "mix_identity")


class Refused(ValueError):
    """The parameters the stage refuses."""


def check_params(iterations, lam, mu):
    """-> (lambda, mu) as float32; raises Refused where lsnFusionSmooth returns -1."""
    lam, mu = np.float32(lam), np.float32(mu)
    if not 1 <= int(iterations) <= 64:
        raise Refused("iterations")
    if not (np.float32(0) < lam <= np.float32(1)):          # NaN fails
        raise Refused("lambda")
    if not (np.float32(-1) <= mu <= np.float32(0)):
        raise Refused("mu")
    return lam, mu


def mix(i):
    """The splitmix64 finaliser of the indices i (any integer array) as uint64."""
    with np.errstate(over="ignore"):
        x = np.asarray(i).astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def open_hash(t, nv, mutant=None):
    """H uint64 [nv] of the valid triangles t (int64 [m, 3], in range and pairwise distinct)."""
    h = np.zeros(nv, np.uint64)
    f = (lambda i: np.asarray(i).astype(np.uint64)) if mutant == "mix_identity" else mix
    with np.errstate(over="ignore"):
        for k in range(3):
            np.add.at(h, t[:, k], f(t[:, (k + 1) % 3]) - f(t[:, (k + 2) % 3]))
    return h


def quantise(xyz, mutant=None):
    with np.errstate(all="ignore"):
        scaled = xyz * SCALE                                           # float32, exact for |c| < 4096
        return (np.floor(scaled) if mutant == "floor" else np.trunc(scaled)).astype(np.int64)


def one_pass(xyz, t, f, pinned, mutant=None):
    """xyz float32 [nv, 3]; t int64 [m, 3], in range and pairwise distinct; f float32; pinned bool [nv].
    -> (xyz' float32 [nv, 3], used triangles, vertices with N == 0)."""
    nv = len(xyz)
    with np.errstate(all="ignore"):
        fine = (np.abs(xyz) < LIMIT).all(axis=1)                       # in float32; NaN and +-inf compare false
    used = fine[t].all(axis=1) if len(t) else np.zeros(0, bool)
    u = t[used]
    if mutant == "gauss_seidel":
        return _gauss_seidel(xyz, u, f, pinned), int(used.sum()), None
    S, N = np.zeros((nv, 3), np.int64), np.zeros(nv, np.int64)
    if mutant == "dedup":
        pairs = np.unique(np.concatenate([u[:, [a, b]] for a in range(3) for b in range(3) if a != b]), axis=0) if len(u) else np.zeros((0, 2), np.int64)
        xyz_ok = np.where(fine[:, None], xyz, np.float32(0))
        np.add.at(S, pairs[:, 0], quantise(xyz_ok, mutant)[pairs[:, 1]])
        np.add.at(N, pairs[:, 0], 1)
    else:
        q = quantise(np.where(fine[:, None], xyz, np.float32(0)), mutant)   # (the corners of used triangles are all fine)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            np.add.at(S, u[:, a], q[u[:, b]] + q[u[:, c]])             # int64 addition wraps
            np.add.at(N, u[:, a], 1 if mutant == "count_one" else 2)
    move = (N > 0) & ~pinned
    out = xyz.copy()
    with np.errstate(all="ignore"):
        m = ((S[move].astype(np.float64) / N[move].astype(np.float64)[:, None]) * 2.0 ** -32).astype(np.float32)
        p = xyz[move]
        d = (m - p).astype(np.float32)
        out[move] = (p + (np.float32(f) * d).astype(np.float32)).astype(np.float32)
    return out, int(used.sum()), int((N == 0).sum())


def _gauss_seidel(xyz, u, f, pinned):
    """The mutant that reads half-updated positions: the vertices in ascending index, each from the positions as they stand."""
    out = xyz.copy()
    for a in range(len(xyz)):
        rows = u[(u == a).any(axis=1)]
        if pinned[a] or not len(rows):
            continue
        others = np.concatenate([r[r != a] for r in rows])
        S = quantise(out[others]).sum(axis=0)
        m = ((S.astype(np.float64) / float(len(others))) * 2.0 ** -32).astype(np.float32)
        d = (m - out[a]).astype(np.float32)
        out[a] = (out[a] + (np.float32(f) * d).astype(np.float32)).astype(np.float32)
    return out


def factors(iterations, lam, mu, mutant=None):
    """The passes' factors in order."""
    lam, mu = check_params(iterations, lam, mu)
    return [f for _ in range(int(iterations)) for f in ((lam,) if mu == 0 or mutant == "no_mu" else (lam, mu))]


def smooth(vertices, offsets, triangles, tri_offsets, iterations, lam, mu, pin_boundary=True, vertex_capacity=None, triangle_capacity=None,
           mutant=None):
    """One tick.  vertices: VERTEX_DTYPE array with at least offsets[-1] entries; offsets, tri_offsets: the tick's rows (n + 1 ints);
    triangles: int32 [m, 3] with at least tri_offsets[-1] rows.  Returns a dict: vertices (VERTEX_DTYPE [nVertices], the colours carried
    over), xyz float32 [nVertices, 3], open bool [nVertices], and the diagnostics used, skipped (both of the last pass), pinned, isolated
    (vertices with N == 0 in the last pass)."""
    assert mutant is None or mutant in MUTANTS, mutant
    fs = factors(iterations, lam, mu, mutant)
    nv, nt = max(0, int(np.asarray(offsets)[-1])), max(0, int(np.asarray(tri_offsets)[-1]))
    if vertex_capacity is not None:
        nv = min(nv, int(vertex_capacity))
    if triangle_capacity is not None:
        nt = min(nt, int(triangle_capacity))
    v = np.asarray(vertices)[:nv].copy()
    xyz = np.stack([v["X"], v["Y"], v["Z"]], axis=1).astype(np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)[:nt].astype(np.int64)
    valid = ((t >= 0) & (t < nv)).all(axis=1) & (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    t = t[valid]
    is_open = open_hash(t, nv, mutant) != 0
    pinned = is_open if pin_boundary and mutant != "no_pin" else np.zeros(nv, bool)
    used = isolated = 0
    for f in fs:
        xyz, used, isolated = one_pass(xyz, t, f, pinned, mutant)
    v["X"], v["Y"], v["Z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return {"vertices": v, "xyz": xyz, "open": is_open, "used": used, "skipped": nt - used, "pinned": int(pinned.sum()), "isolated": isolated}
