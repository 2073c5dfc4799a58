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


def k_distance(pts, k, rules=None, pool=None):
    """KNNeighbors' kDistance (filter.cpp:19-34): the k-th smallest squared distance of every point to the cloud, chunked brute force;
    FLT_MAX for every point of a cloud of fewer than k points (KNNResultSet::init writes dists[k-1], nothing overwrites it).
    rules (names of RULES) / pool: a neighbouring wrong rule instead (wrong_k_distance below); without them, exactly the above."""
    if rules or pool is not None:
        return wrong_k_distance(pts, k, rules, pool)
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


def keep_mask(pts, k, max_dist, brute_limit=8000, rules=None, pool=None):
    """The points filter() keeps (filter.cpp:40-58): kDistance > distThreshold removes.  Small clouds: the order statistic itself; larger
    ones: its count form, #{d^2 <= thr} >= k (the same set: the k-th smallest is > thr iff fewer than k are <= thr).
    rules (names of RULES) / pool: a neighbouring wrong rule instead (wrong_keep_mask below); without them, exactly the above."""
    if rules or pool is not None:
        return wrong_keep_mask(pts, k, max_dist, rules, pool)
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


# ---- neighbouring wrong rules (tests/test_outlier_boundary_ref.py: every one of them is told apart from the filter by a named case) ----

RULES = {
    "lt_thr": "a neighbour needs d^2 < thr, not <=",
    "self_not_counted": "the point itself is no neighbour of its own",
    "duplicates_once": "points at one position count once",
    "thr_not_squared": "thr = maxDist",
    "thr_double": "thr = maxDist^2 kept in double",
    "d2_double": "d^2: float differences, squared and summed in double",
    "d2_right_to_left": "d^2 = d0*d0 + (d1*d1 + d2*d2)",
    "d2_fma": "d^2 = fma(d2, d2, d0*d0 + d1*d1)",
    "k_plus_1": "k + 1 neighbours asked for",
    "small_le_k": "a block of n <= k points is a small block",
    "small_removed": "a small block is always removed",
    "small_kept": "a small block is always kept",
    "scope_tick": "neighbours from every sensor of the tick",
    "scope_batch": "neighbours from every sensor of every tick of the batch",
}


def _wrong_dist2(q, p, rules):
    d0 = q[:, None, 0] - p[None, :, 0]
    d1 = q[:, None, 1] - p[None, :, 1]
    d2 = q[:, None, 2] - p[None, :, 2]
    if "d2_double" in rules:
        d0, d1, d2 = d0.astype(np.float64), d1.astype(np.float64), d2.astype(np.float64)
        return d0 * d0 + d1 * d1 + d2 * d2
    if "d2_right_to_left" in rules:
        return d0 * d0 + (d1 * d1 + d2 * d2)
    if "d2_fma" in rules:   # the product of two floats is exact in double; the sum is rounded to double and then to float
        return (d2.astype(np.float64) * d2.astype(np.float64) + (d0 * d0 + d1 * d1).astype(np.float64)).astype(np.float32)
    return d0 * d0 + d1 * d1 + d2 * d2


def wrong_k_distance(pts, k, rules=None, pool=None):
    """k_distance under the rules of `rules`; pool = (points, first): the neighbours come from `points`, of which pts is the slice that
    starts at `first` (the scope rules, filter_batch below).  float64 under d2_double."""
    rules = set(rules or ())
    assert rules <= set(RULES), rules - set(RULES)
    pts = xyz(pts)
    cloud, first = (pts, 0) if pool is None else (xyz(pool[0]), int(pool[1]))
    n = len(pts)
    k = k + 1 if "k_plus_1" in rules else k
    out = np.full(n, FLT_MAX, dtype=np.float64 if "d2_double" in rules else np.float32)
    if n == 0 or (n <= k if "small_le_k" in rules else n < k):
        return out
    d = _wrong_dist2(pts, cloud, rules).astype(out.dtype)
    big = np.asarray(np.inf, dtype=out.dtype)
    if "duplicates_once" in rules:
        _, firsts = np.unique(cloud, axis=0, return_index=True)
        gone = np.ones(len(cloud), bool)
        gone[firsts] = False
        d[:, gone] = big
    if "self_not_counted" in rules:
        d[np.arange(n), first + np.arange(n)] = big
    if d.shape[1] < k:
        return out
    kd = np.partition(d, k - 1, axis=1)[:, k - 1]
    return np.where(np.isinf(kd) & ~np.isinf(out), out, kd).astype(out.dtype)   # fewer than k candidates left: init's FLT_MAX


def wrong_keep_mask(pts, k, max_dist, rules=None, pool=None):
    rules = set(rules or ())
    assert rules <= set(RULES), rules - set(RULES)
    pts = xyz(pts)
    n = len(pts)
    if k <= 0 or max_dist <= 0 or n == 0:
        return np.ones(n, dtype=bool)
    thr = threshold(max_dist)
    if "thr_not_squared" in rules:
        thr = np.float32(max_dist)
    if "thr_double" in rules:
        thr = np.float64(np.float32(max_dist)) ** 2
    kk = k + 1 if "k_plus_1" in rules else k
    if n <= kk if "small_le_k" in rules else n < kk:
        if "small_removed" in rules or "small_kept" in rules:
            return np.full(n, "small_kept" in rules)
    kd = wrong_k_distance(pts, k, rules, pool)
    return kd < thr if "lt_thr" in rules else ~(kd > thr)


def filter_batch(ticks, k, max_dist, rules=None, brute_limit=8000):
    """ticks[t][s]: the (n, 3) block of sensor s in tick t.  The keep mask of every block: every block on its own (keep_mask), unless
    `rules` says otherwise."""
    rules = set(rules or ())
    out = []
    everything = [b for tick in ticks for b in tick]
    for t, tick in enumerate(ticks):
        row = []
        for s, b in enumerate(tick):
            pool = None
            if "scope_batch" in rules:
                before = sum(len(x) for tk in ticks[:t] for x in tk) + sum(len(x) for x in tick[:s])
                pool = (np.concatenate([xyz(x) for x in everything]), before)
            elif "scope_tick" in rules:
                pool = (np.concatenate([xyz(x) for x in tick]), sum(len(x) for x in tick[:s]))
            only_scope = rules <= {"scope_tick", "scope_batch"}
            row.append(keep_mask(b, k, max_dist, brute_limit) if not rules else
                       keep_mask(b, k, max_dist, rules=rules - {"scope_tick", "scope_batch"} if not only_scope else None, pool=pool))
        out.append(row)
    return out


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
