"""Mesh level of detail (lsnFusionSimplify) restated in numpy: the definition the kernels are held to bit for bit.

The reference has no decimation; nothing here is pinned to it.  inv = float32(1) / float32(cell); per axis q = floor(c * inv) in float32;
an axis is in range iff q is finite and -2^20 <= q < 2^20 (compared in float); a vertex with three axes in range has the key
(qx + 2^20) | (qy + 2^20) << 21 | (qz + 2^20) << 42, every other vertex is a cell of its own.  The vertex of lowest index represents its
cell and keeps its bytes; representatives leave in ascending index; triangles are remapped, dropped when two new indices are equal or an
index was out of range, and keep their order.  cell <= 0 or NaN copies."""
import numpy as np

from livescan3d_amd import native

LIM = np.float32(2 ** 20)


def cell_keys(vertices, cell):
    """-> (key uint64 [n], clustered bool [n]) of a VERTEX_DTYPE array; the key of an unclustered vertex is meaningless."""
    with np.errstate(all="ignore"):
        inv = np.float32(1.0) / np.float32(cell)
        key = np.zeros(len(vertices), np.uint64)
        ok = np.ones(len(vertices), bool)
        for axis, name in enumerate("XYZ"):
            q = np.floor((vertices[name].astype(np.float32) * inv).astype(np.float32))
            in_range = np.isfinite(q) & (q >= -LIM) & (q < LIM)
            ok &= in_range
            key |= (np.where(in_range, q, 0).astype(np.int64) + 2 ** 20).astype(np.uint64) << np.uint64(21 * axis)
    return key, ok


def simplify(vertices, offsets, triangles, tri_offsets, cell, vertex_capacity=None, triangle_capacity=None):
    """One tick.  vertices: VERTEX_DTYPE array with at least offsets[-1] entries; offsets: the tick's row (n + 1 ints); triangles: int32
    [m, 3] with at least tri_offsets[-1] rows, or None (points only; tri_offsets is then ignored).  Returns a dict: vertices, offsets,
    triangles, tri_offsets (None in points mode), remap int32 [nVertices], cells, unclustered, dropped_triangles."""
    offsets = np.asarray(offsets, np.int64)
    nv = max(0, int(offsets[-1]))
    if vertex_capacity is not None:
        nv = min(nv, int(vertex_capacity))
    v = np.asarray(vertices)[:nv]
    points = triangles is None
    if not points:
        tri_offsets = np.asarray(tri_offsets, np.int64)
        nt = max(0, int(tri_offsets[-1]))
        if triangle_capacity is not None:
            nt = min(nt, int(triangle_capacity))
        t = np.asarray(triangles, np.int32).reshape(-1, 3)[:nt]
    cell = np.float32(cell)
    if not cell > 0:   # <= 0 or NaN: off
        return {"vertices": v.copy(), "offsets": offsets.astype(np.int32), "triangles": None if points else t.copy(),
                "tri_offsets": None if points else tri_offsets.astype(np.int32), "remap": np.arange(nv, dtype=np.int32), "cells": nv,
                "unclustered": 0, "dropped_triangles": 0}
    key, ok = cell_keys(v, cell)
    rep = np.arange(nv, dtype=np.int64)
    idx = np.flatnonzero(ok)
    if len(idx):
        _, first, inverse = np.unique(key[idx], return_index=True, return_inverse=True)   # first: the lowest position of every key
        rep[idx] = idx[first[inverse.ravel()]]
    kept = rep == np.arange(nv)
    below = np.concatenate([[0], np.cumsum(kept)])        # below[j]: kept vertices of index < j
    remap = (below[rep] if nv else np.zeros(0, np.int64)).astype(np.int32)
    out = {"vertices": v[kept].copy(), "offsets": below[np.clip(offsets, 0, nv)].astype(np.int32), "remap": remap, "cells": int(kept.sum()),
           "unclustered": int((~ok).sum()), "triangles": None, "tri_offsets": None, "dropped_triangles": 0}
    if not points:
        valid = ((t >= 0) & (t < nv)).all(axis=1)
        new = remap[np.where(valid[:, None], t, 0)] if nv else np.zeros((len(t), 3), np.int32)
        keep = valid & (new[:, 0] != new[:, 1]) & (new[:, 1] != new[:, 2]) & (new[:, 0] != new[:, 2])
        tbelow = np.concatenate([[0], np.cumsum(keep)])
        out["triangles"] = new[keep].astype(np.int32)
        out["tri_offsets"] = tbelow[np.clip(tri_offsets, 0, nt)].astype(np.int32)
        out["dropped_triangles"] = int(nt - keep.sum())
    return out


def cloud(xyz, colors=None):
    """A VERTEX_DTYPE array from [n, 3] coordinates (colour: the index, so that every vertex has bytes of its own)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    v = np.zeros(len(xyz), native.VERTEX_DTYPE)
    v["X"], v["Y"], v["Z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    raw = v.view(np.uint8).reshape(-1, 16)
    raw[:, :4] = ((np.arange(len(xyz), dtype=np.uint64) + 1) * 2654435761 % 2 ** 32).astype("<u4").view(np.uint8).reshape(-1, 4) if colors is None \
        else np.asarray(colors, np.uint8).reshape(-1, 4)
    return v
