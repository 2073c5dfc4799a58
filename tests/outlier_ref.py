"""numpy restatement of LiveScanClient's outlier filter (test infrastructure), cited against the reference:

  filter()          src/LiveScanClient/filter.cpp:36-81
  KNNeighbors       src/LiveScanClient/filter.cpp:19-34 (nanoflann knnSearch over the same cloud: the point itself counts, at 0)
  kdtree_distance   include/LiveScanClient/filter.h:38-45 (d = query - point; d0*d0 + d1*d1 + d2*d2, float, left to right)

Per sensor block, as the library scopes it: filter_rig() gives the masked depth maps the GPU path fuses again.
float32 numpy arithmetic rounds every operation to float32 and never contracts, like the reference's /fp:precise build."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
CHUNK = 512


def xyz(v):
    """(n, 3) float32 positions of a VERTEX_DTYPE array or of an (n, 3) array."""
    if getattr(v, "dtype", None) is not None and v.dtype.names:
        return np.stack([v["X"], v["Y"], v["Z"]], axis=1).astype(np.float32)
    return np.asarray(v, dtype=np.float32).reshape(-1, 3)


def dist2(q, p):
    """kdtree_distance (filter.h:40-44) of every query row against every point row: (m, n) float32."""
    d0 = q[:, None, 0] - p[None, :, 0]
    d1 = q[:, None, 1] - p[None, :, 1]
    d2 = q[:, None, 2] - p[None, :, 2]
    return d0 * d0 + d1 * d1 + d2 * d2


def threshold(max_dist):
    """distThreshold = pow(maxDist, 2) stored in a float (filter.cpp:53): the double square of a float is exact, so it rounds to the float
    product."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(np.float32(max_dist) * np.float32(max_dist))


def k_distance(pts, k):
    """KNNeighbors' kDistance (filter.cpp:19-34): the k-th smallest squared distance of every point to the cloud, chunked brute force;
    FLT_MAX for every point of a cloud of fewer than k points (KNNResultSet::init writes dists[k-1], nothing overwrites it)."""
    pts = xyz(pts)
    n = len(pts)
    out = np.full(n, FLT_MAX, dtype=np.float32)
    if n < k:
        return out
    for c in range(0, n, CHUNK):
        out[c:c + CHUNK] = np.partition(dist2(pts[c:c + CHUNK], pts), k - 1, axis=1)[:, k - 1]
    return out


def neighbour_counts(pts, thr, idx=None):
    """#{j : kdtree_distance(p_i, p_j) <= thr} for the points idx (default all), exact.  Only points within w of p_i along x can pass,
    w = sqrt(thr) (1 + 2^-20) + 2^-70 (the bound outlier.hip's ol_cell proves), so each query is held against the points of its x window."""
    pts = xyz(pts)
    idx = np.arange(len(pts)) if idx is None else np.asarray(idx, dtype=np.int64)
    out = np.zeros(len(idx), dtype=np.int64)
    if len(idx) == 0:
        return out
    thr = np.float32(thr)
    if np.isnan(thr):
        return out
    w = float(np.sqrt(np.float64(thr))) * (1 + 2.0 ** -20) + 2.0 ** -70
    order = np.argsort(pts[:, 0], kind="stable")
    xs = pts[order, 0].astype(np.float64)
    perm = np.argsort(pts[idx, 0], kind="stable")
    c = 0
    while c < len(perm):
        step = CHUNK
        while True:
            pos = perm[c:c + step]
            q = pts[idx[pos]]
            lo = np.searchsorted(xs, float(q[:, 0].min()) - w, "left")
            hi = np.searchsorted(xs, float(q[:, 0].max()) + w, "right")
            if step <= 8 or (hi - lo) * len(pos) <= 8_000_000:
                break
            step //= 4
        out[pos] = (dist2(q, pts[order[lo:hi]]) <= thr).sum(axis=1)
        c += step
    return out


def keep_mask(pts, k, max_dist, brute_limit=8000):
    """The points filter() keeps (filter.cpp:40-58): kDistance > distThreshold removes.  Small clouds: the order statistic itself; larger
    ones: its count form, #{d^2 <= thr} >= k (the same set: the k-th smallest is > thr iff fewer than k are <= thr)."""
    pts = xyz(pts)
    n = len(pts)
    if k <= 0 or max_dist <= 0 or n == 0:   # :40-41 (a NaN maxDist passes this test)
        return np.ones(n, dtype=bool)
    thr = threshold(max_dist)
    if n < k:
        return np.full(n, not (FLT_MAX > thr))
    if n <= brute_limit:
        return ~(k_distance(pts, k) > thr)
    if np.isnan(thr):
        return np.ones(n, dtype=bool)
    return neighbour_counts(pts, thr) >= k


def filter(vertices, colors, k, max_dist):
    """filter() itself (filter.cpp:36-81): (kept vertices, their colours, changedVerticesMap as a dict)."""
    keep = keep_mask(vertices, k, max_dist)
    changed = {-1: -1}
    if k <= 0 or max_dist <= 0:
        return vertices, colors, changed
    new = np.cumsum(keep) - 1
    for i in range(len(keep)):
        changed[i] = int(new[i]) if keep[i] else -1
    return vertices[keep], colors[keep], changed


def filter_vertices(verts, k, max_dist):
    """generateVerticesFromDepthMap's cloud (VERTEX_DTYPE) filtered: the survivors in order, colours with them."""
    return verts[keep_mask(verts, k, max_dist)]


def sensor_frames(rig):
    """Per sensor: (depth (h, w) u16, rgb (h, w, 3) u8, intr7, wt12)."""
    dm = rig.depth_maps.view("<u2")
    out, p = [], 0
    for i in range(rig.n):
        w, h = int(rig.widths[i]), int(rig.heights[i])
        out.append((dm[p:p + w * h].reshape(h, w), rig.depth_colors[3 * p:3 * (p + w * h)].reshape(h, w, 3),
                    rig.intr[7 * i:7 * i + 7], rig.wt[12 * i:12 * i + 12]))
        p += w * h
    return out


def filter_rig(rig, k, max_dist, orc):
    """The masked depth maps of a merge call with the filter on: every sensor's cloud (orc.create_vertices) filtered
    on its own, depth 0 at the pixels of removed vertices.  Returns (depth maps as a uint8 view like rig.depth_maps, [removed flags per
    sensor's vertex])."""
    maps, removed = [], []
    for depth, rgb, intr, wt in sensor_frames(rig):
        verts, v2p, _ = orc.create_vertices(depth, rgb, intr, wt, rig.bounds, want_maps=True)
        keep = keep_mask(verts, k, max_dist)
        d = depth.copy().ravel()
        d[v2p[~keep]] = 0
        maps.append(d)
        removed.append(~keep)
    dm = np.concatenate(maps).astype("<u2") if maps else np.zeros(0, "<u2")
    return dm.view(np.uint8), removed


def masked_rig(rig, masked_maps):
    """A copy of the rig with other depth maps."""
    import copy
    r = copy.copy(rig)
    r.depth_maps = np.ascontiguousarray(masked_maps)
    return r
