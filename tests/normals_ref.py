"""Vertex normals of the merged mesh (lsnFusionNormals) restated in numpy: the definition the kernels are held to
bit for bit.

The reference computes no normals; nothing here is pinned to it.  Face vector of a triangle (i0, i1, i2): u = p2 - p0, v = p1 - p0,
f = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x), every float32 operation rounded on its own.  The triangle is used iff its
indices are in [0, nVertices) and |fx|, |fy|, |fz| < 4096 (in float32; NaN and inf fail), else skipped.  q = int64(trunc(f * 2^40)), exact;
S[i] += q at i0, i1, i2 in int64 with wrap-around.  S == (0, 0, 0): the normal is (+0, +0, +0); else s = float32(S) (round to nearest
even), len = sqrt((s.x s.x + s.y s.y) + s.z s.z), n = s / len, all float32."""
import numpy as np

LIMIT = np.float32(4096.0)
SCALE = np.float32(2.0 ** 40)


def face_vectors(xyz, t):
    """float32 [m, 3]: (p2 - p0) x (p1 - p0) of the triangles t (int [m, 3], indices in range) over the positions xyz (float32 [n, 3])."""
    with np.errstate(all="ignore"):
        p0, p1, p2 = xyz[t[:, 0]], xyz[t[:, 1]], xyz[t[:, 2]]
        u, v = p2 - p0, p1 - p0
        return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]],
                        axis=1).astype(np.float32)


def normals(vertices, offsets, triangles, tri_offsets, vertex_capacity=None, triangle_capacity=None):
    """One tick.  vertices: VERTEX_DTYPE array with at least offsets[-1] entries; offsets, tri_offsets: the tick's rows (n + 1 ints);
    triangles: int32 [m, 3] with at least tri_offsets[-1] rows.  Returns a dict: normals float32 [nVertices, 3], sums int64 [nVertices, 3],
    used, skipped, zero_normals."""
    nv, nt = max(0, int(np.asarray(offsets)[-1])), max(0, int(np.asarray(tri_offsets)[-1]))
    if vertex_capacity is not None:
        nv = min(nv, int(vertex_capacity))
    if triangle_capacity is not None:
        nt = min(nt, int(triangle_capacity))
    v = np.asarray(vertices)[:nv]
    xyz = np.stack([v["X"], v["Y"], v["Z"]], axis=1).astype(np.float32).reshape(-1, 3)
    t = np.asarray(triangles, np.int32).reshape(-1, 3)[:nt].astype(np.int64)
    in_range = ((t >= 0) & (t < nv)).all(axis=1)
    t = t[in_range]
    f = face_vectors(xyz, t) if len(t) else np.zeros((0, 3), np.float32)
    with np.errstate(all="ignore"):
        ok = (np.abs(f) < LIMIT).all(axis=1)                          # in float32; NaN and +-inf compare false
        q = np.trunc(f[ok] * SCALE).astype(np.int64)                 # |f| < 2^12: product and conversion are exact
    sums = np.zeros((nv, 3), np.int64)
    for k in range(3):
        np.add.at(sums, t[ok][:, k], q)                               # int64 addition wraps
    zero = (sums == 0).all(axis=1)
    with np.errstate(all="ignore"):
        s = sums.astype(np.float32)                                   # round to nearest even
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        n = (s / length[:, None]).astype(np.float32)
    n[zero] = 0.0
    return {"normals": n, "sums": sums, "used": int(ok.sum()), "skipped": int(nt - ok.sum()), "zero_normals": int(zero.sum())}
