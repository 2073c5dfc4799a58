"""The fragment filter (lsnFusionFragments) restated in numpy: the definition the kernels are held to bit for bit.

The reference has no such step; nothing here is pinned to it.  A triangle is valid iff its three indices lie in [0, nVertices); a valid
triangle (i0, i1, i2) joins i0-i1 and i1-i2; label[v] is the lowest vertex index of v's connected component; a component's size is the
number of vertices that carry its label; a vertex is kept iff size[label[v]] >= min_vertices.  Kept vertices leave in ascending index,
valid triangles of kept components are remapped and keep their order.  min_vertices <= 1 copies.  A plain union-find over integer arrays."""
import numpy as np


def labels_of(nv, triangles):
    """label int64 [nv] of the graph of `triangles` (int [m, 3]; invalid ones join nothing): union-find, the lower root wins."""
    parent = list(range(nv))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    for i0, i1, i2 in np.asarray(triangles, np.int64).reshape(-1, 3).tolist():
        if 0 <= i0 < nv and 0 <= i1 < nv and 0 <= i2 < nv:
            union(i0, i1)
            union(i1, i2)
    return np.array([find(v) for v in range(nv)], np.int64).reshape(nv)


def fragments(vertices, offsets, triangles, tri_offsets, min_vertices, vertex_capacity=None, triangle_capacity=None):
    """One tick.  vertices: VERTEX_DTYPE array with at least offsets[-1] entries; offsets: the tick's row (n + 1 ints); triangles: int32
    [m, 3] with at least tri_offsets[-1] rows.  Returns a dict: vertices, offsets, triangles, tri_offsets, remap int32 [nVertices], labels
    int32 [nVertices] (None when off), components, removed_components, removed_vertices, dropped_triangles."""
    offsets = np.asarray(offsets, np.int64)
    tri_offsets = np.asarray(tri_offsets, np.int64)
    nv, nt = max(0, int(offsets[-1])), max(0, int(tri_offsets[-1]))
    if vertex_capacity is not None:
        nv = min(nv, int(vertex_capacity))
    if triangle_capacity is not None:
        nt = min(nt, int(triangle_capacity))
    v = np.asarray(vertices)[:nv]
    t = np.asarray(triangles, np.int32).reshape(-1, 3)[:nt]
    if int(min_vertices) <= 1:   # off
        return {"vertices": v.copy(), "offsets": offsets.astype(np.int32), "triangles": t.copy(), "tri_offsets": tri_offsets.astype(np.int32),
                "remap": np.arange(nv, dtype=np.int32), "labels": None, "components": 0, "removed_components": 0, "removed_vertices": 0,
                "dropped_triangles": 0}
    label = labels_of(nv, t)
    size = np.bincount(label, minlength=nv) if nv else np.zeros(0, np.int64)
    kept = size[label] >= int(min_vertices) if nv else np.zeros(0, bool)
    below = np.concatenate([[0], np.cumsum(kept)])        # below[j]: kept vertices of index < j
    remap = np.where(kept, below[:-1], -1).astype(np.int32)
    roots = label == np.arange(nv)
    valid = ((t >= 0) & (t < nv)).all(axis=1)
    keep_t = valid.copy()
    keep_t[valid] = kept[t[valid, 0]]
    tbelow = np.concatenate([[0], np.cumsum(keep_t)])
    return {"vertices": v[kept].copy(), "offsets": below[np.clip(offsets, 0, nv)].astype(np.int32),
            "triangles": remap[t[keep_t]].astype(np.int32).reshape(-1, 3), "tri_offsets": tbelow[np.clip(tri_offsets, 0, nt)].astype(np.int32),
            "remap": remap, "labels": label.astype(np.int32), "components": int(roots.sum()),
            "removed_components": int((roots & ~kept).sum()), "removed_vertices": int(nv - kept.sum()),
            "dropped_triangles": int(nt - keep_t.sum())}
