"""A second restatement of the colour blend (tests/color_blend_ref.py is the definition) in plain Python: a triple loop over ticks,
vertices and sensors, to cross-check the numpy form on the hand-made rigs.  TEST INFRASTRUCTURE ONLY; slow by design.
Float32 arithmetic goes through numpy float32 scalars (one rounding per operation); the confidence maps are color_ref_py's.

blend_ticks(ticks, orc, depth_tol, min_confidence, rules=...) computes the neighbouring WRONG rule instead of the true one at one
decision (RULES: name -> what it does): the mutants tests/test_color_blend_ref.py uses to show that a rig decides an output.  Without
rules nothing changes."""
import math

import numpy as np

from tests import color_ref_py

F = np.float32

RULES = {
    "tol_le": "|d1 - d2| <= depth_tol", "no_abs": "d1 - d2 < depth_tol, without the absolute value",
    "conf_gt": "partner confidence > min_confidence", "conf_ge_m1": "partner confidence >= min_confidence - 1",
    "own_gated": "the own term takes part only at confidence >= min_confidence",
    "no_vertex_read": "a pixel with depth but no vertex contributes C_in[-1]",
    "project_floor": "x and y are rounded down, not truncated", "edge_inclusive": "x == w and y == h count as the last column and row",
    "no_d1_test": "d1 == 0 is not rejected", "cvt_saturates": "double -> int saturates and gives 0 for NaN (v_cvt_i32_f64)",
    "d_wraps": "d1 is cut to 16 bits, not clamped at 65535",
    "lower_only": "only the sensors i < j are partners",
    "gauss_seidel": "in place, sensor by sensor: a later sensor reads the colours the earlier ones were given",
    "raw_colors": "a partner's colour is sampled from its colour map, not from the vertices handed in",
    "tick0_index": "every tick uses tick 0's pixel -> vertex maps and confidence maps",
    "no_half": "floor(sum / W), without the half", "half_ceil": "the half is ceil(W / 2)",
    "sum_16bit": "the weighted sums are kept in 16 bits",
    "min0_off": "min_confidence < 1 switches the stage off", "alpha_255": "the alpha byte of a blended vertex becomes 255",
}
_RULES = frozenset()


def _on(name):
    return name in _RULES


def _to_int(v, floor=False):
    """(int) of a Python float (double) on x64."""
    if _on("cvt_saturates"):
        return 0 if math.isnan(v) else int(min(max(v, -2147483648.0), 2147483647.0))
    if math.isnan(v) or not (-2147483649.0 < v < 2147483648.0):
        return -2 ** 31
    return math.floor(v) if floor and _on("project_floor") else int(v)      # truncates toward zero


def _projection(X, Y, Z, intr, wt):
    t = [-F(wt[0]), -F(wt[1]), -F(wt[2])]
    R = [[F(wt[3 + 3 * c + r]) for c in range(3)] for r in range(3)]      # transposed
    X, Y, Z = F(X), F(Y), F(Z)
    with np.errstate(all="ignore"):
        tx = X * R[0][0] + Y * R[0][1] + Z * R[0][2] + t[0]
        ty = X * R[1][0] + Y * R[1][1] + Z * R[1][2] + t[1]
        tz = X * R[2][0] + Y * R[2][1] + Z * R[2][2] + t[2]
        cx, cy, fx, fy = (F(intr[k]) for k in range(4))
        x = _to_int(float((tx * fx) / tz + cx) + 0.5, floor=True)
        y = _to_int(float(cy - (ty * fy) / tz) + 0.5, floor=True)
        d = max(0, _to_int(float(tz * F(1000.0))))
    return x, y, (d & 0xFFFF if _on("d_wraps") else min(d, 65535))


def _sensors(rig, orc):
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2")
    dc = np.ascontiguousarray(rig.depth_colors)
    S, po = [], 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        depth = dm[po:po + w * h].reshape(h, w)
        rgb = dc[3 * po:3 * (po + w * h)].reshape(h, w, 3)
        verts, v2p, p2v = orc.create_vertices(depth, rgb, rig.intr[7 * s:7 * s + 7], rig.wt[12 * s:12 * s + 12], rig.bounds, want_maps=True)
        S.append(dict(w=w, h=h, d=[int(v) for v in depth.ravel()], conf=color_ref_py.confidence(depth), verts=verts, v2p=[int(v) for v in v2p],
                      p2v=[int(v) for v in p2v], intr=rig.intr[7 * s:7 * s + 7], wt=rig.wt[12 * s:12 * s + 12],
                      raw=[tuple(int(c) for c in px) for px in rgb.reshape(-1, 3)]))
        po += w * h
    return S


def blend_ticks(ticks, orc, depth_tol, min_confidence, verts=None, rules=()):
    """ticks: the rigs of one plan's ticks; verts: per tick the cloud to blend (None: as fused).  Same result per tick as
    color_blend_ref.blend: [(vertices, diagnostics)].  rules: names of RULES to compute wrongly."""
    global _RULES
    assert set(rules) <= set(RULES), rules
    _RULES = frozenset(rules)
    try:
        first = None
        out = []
        for k, rig in enumerate(ticks):
            S = _sensors(rig, orc)
            first = S if first is None else first
            out.append(_blend(S, first if _on("tick0_index") else S, depth_tol, min_confidence, None if verts is None else verts[k]))
        return out
    finally:
        _RULES = frozenset()


def _blend(S, index, depth_tol, min_confidence, verts):
    """S: the tick's sensors; index: the sensors whose maps (p2v, conf) are read (S itself, but for one mutant)."""
    n = len(S)
    if n > 32:
        raise ValueError(f"at most 32 sensors (the rig has {n})")
    off = [0]
    for s in S:
        off.append(off[-1] + len(s["verts"]))
    cur = np.concatenate([s["verts"] for s in S]) if verts is None else np.array(verts, copy=True)
    assert len(cur) == off[-1]
    diag = {"blended": np.zeros(n, np.int32), "partners": np.zeros(n, np.int64), "abs_change": np.zeros(n, np.int64)}
    if depth_tol <= 0 or min_confidence > 20 or n == 1 or (_on("min0_off") and min_confidence < 1):
        return cur, diag
    mc = max(min_confidence, 1)
    c_in = [(int(v["R"]), int(v["G"]), int(v["B"])) for v in cur]
    read = list(c_in) if _on("gauss_seidel") else c_in      # what a partner's colour is read from
    mask = 0xFFFF if _on("sum_16bit") else -1
    for j in range(n):
        new = {}
        for g in range(off[j], off[j + 1]):
            vert = cur[g]
            w0 = index[j]["conf"][S[j]["v2p"][g - off[j]]]
            if _on("own_gated") and w0 < mc:
                w0 = 0
            W, num, partners = w0, [w0 * c for c in read[g]], 0
            for i in range(n):
                if i == j or (_on("lower_only") and i > j):
                    continue
                a = S[i]
                x, y, d1 = _projection(vert["X"], vert["Y"], vert["Z"], a["intr"], a["wt"])
                if _on("edge_inclusive"):
                    x, y = (a["w"] - 1 if x == a["w"] else x), (a["h"] - 1 if y == a["h"] else y)
                if x < 0 or x >= a["w"] or y < 0 or y >= a["h"]:
                    continue
                if d1 == 0 and not _on("no_d1_test"):
                    continue
                q = x + y * a["w"]
                d2 = a["d"][q]
                diff = d1 - d2 if _on("no_abs") else abs(d1 - d2)
                if d2 <= 0 or not (diff <= depth_tol if _on("tol_le") else diff < depth_tol):
                    continue
                v = index[i]["p2v"][q]
                if v < 0 and not _on("no_vertex_read"):
                    continue
                w = index[i]["conf"][q]
                if not (w > mc if _on("conf_gt") else w >= mc - 1 if _on("conf_ge_m1") else w >= mc):
                    continue
                col = a["raw"][q] if _on("raw_colors") else read[(off[i] + v) % len(read)]
                W += w
                num = [(s + w * c) & mask if mask > 0 else s + w * c for s, c in zip(num, col)]
                partners += 1
            if partners and W > 0:
                half = 0 if _on("no_half") else (W + 1) // 2 if _on("half_ceil") else W // 2
                new[g] = tuple(min(255, (s + half) // W) for s in num)      # (the true mean never exceeds 255: only a mutant's can)
                diag["blended"][j] += 1
                diag["partners"][j] += partners
        for g, col in new.items():
            diag["abs_change"][j] += sum(abs(a - b) for a, b in zip(col, c_in[g]))
            cur[g]["R"], cur[g]["G"], cur[g]["B"] = col
            if _on("alpha_255"):
                cur[g]["A"] = 255
            if _on("gauss_seidel"):
                read[g] = col
    return cur, diag
