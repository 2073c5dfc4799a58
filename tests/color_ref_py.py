"""A second restatement of the colour transfer in plain Python loops, written after the reference's own control flow (frontier lists,
per-vertex loops), to cross-check tests/color_ref.py on small rigs.  TEST INFRASTRUCTURE ONLY; slow by design.
Float32 arithmetic goes through numpy float32 scalars (one rounding per operation, as the reference's /fp:precise build).

color_transfer(rig, orc, rules=...) computes the neighbouring WRONG rule instead of the true one at one decision (RULES: name ->
what it does): the mutants tests/test_color_boundary_ref.py uses to show that a boundary rig decides an output.  Without rules
nothing changes."""
import math

import numpy as np

F = np.float32

RULES = {
    "seed_gt_19": "seed test |d - neighbour| > 19", "seed_gt_21": "seed test |d - neighbour| > 21",
    "bfs_lt_19": "BFS step |d - neighbour| < 19", "bfs_lt_21": "BFS step |d - neighbour| < 21",
    "bfs_one_sweep_less": "the BFS stops at level 18 (level 19 is never handed out)",
    "border_low_visited": "the BFS visits x == 0 and y == 0", "border_high_skipped": "the BFS skips x == w - 1 and y == h - 1",
    "cov_lt_19": "coverage: |d1 - d2| < 19", "cov_lt_21": "coverage: |d1 - d2| < 21",
    "smp_lt_19": "samples: |d1 - d2| < 19", "smp_lt_21": "samples: |d1 - d2| < 21",
    "conf_i_ge_4": "confidence of the projected pixel of i >= 4", "conf_i_ge_6": "confidence of the projected pixel of i >= 6",
    "conf_j_ge_4": "confidence of j's own pixel >= 4", "conf_j_ge_6": "confidence of j's own pixel >= 6",
    "coverage_gt_99": "a pair needs coverage > 99", "coverage_gt_101": "a pair needs coverage > 101",
    "first_branch_last_tie": "first branch: the last of equal coverages wins", "second_branch_last_tie": "second branch: the last of equal coverages wins",
    "pair_sorted": "a chosen pair is stored as (min, max)", "first_branch_falls_through": "the second branch runs whenever the first found nothing above 100",
    "bit_31_lost": "sensor 31 is never marked assigned (1 << 31 of a signed int)",
    "smp_d1_test": "samples: d1 == 0 is rejected as in the coverage", "cov_no_d1_test": "coverage: d1 == 0 is not rejected",
    "project_floor": "x and y are rounded down, not truncated", "edge_inclusive": "x == w and y == h count as the last column and row",
    "cvt_saturates": "double -> int saturates and gives 0 for NaN (v_cvt_i32_f64)", "d_wraps": "d is cut to 16 bits, not clamped at 65535",
    "fold_tail_dropped": "the deviation sums stop at the last multiple of 8 samples", "empty_scale_0": "an empty sample set gives scale 0",
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
    return math.floor(v) if floor and _on("project_floor") else int(v)   # truncates toward zero


def confidence(depth):
    h, w = depth.shape
    dm = [int(v) for v in depth.ravel()]
    conf = [20] * (w * h)
    shift_x = [-1, 0, 1, -1, 1, -1, 0, 1]
    shift_y = [-1, -1, -1, 0, 0, 1, 1, 1]
    seed_thr = 19 if _on("seed_gt_19") else 21 if _on("seed_gt_21") else 20
    bfs_thr = 19 if _on("bfs_lt_19") else 21 if _on("bfs_lt_21") else 20
    low = -1 if _on("border_low_visited") else 0
    wh, hh = (w - 1, h - 1) if _on("border_high_skipped") else (w, h)
    last = 18 if _on("bfs_one_sweep_less") else 20
    pos = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            p = y * w + x
            if dm[p] == 0:
                conf[p] = 0
                continue
            for s in range(8):
                q = x + shift_x[s] + (y + shift_x[s]) * w   # sic: shift_x in the row offset
                if abs(dm[p] - dm[q]) > seed_thr or dm[q] == 0:
                    pos.append((x, y))
                    conf[p] = 1
                    break
    max_et = 1
    while pos and max_et != last:
        new = []
        for x, y in pos:
            d = dm[x + y * w]
            for s in range(8):
                nx, ny = x + shift_x[s], y + shift_y[s]
                if nx <= low or ny <= low or nx >= wh or ny >= hh:
                    continue
                q = nx + ny * w
                if abs(d - dm[q]) < bfs_thr and conf[q] == 20 and dm[q] != 0:
                    conf[q] = max_et + 1
                    new.append((nx, ny))
        pos = new
        max_et += 1
    return conf


def projection(v, intr, wt):
    t = [-F(wt[0]), -F(wt[1]), -F(wt[2])]
    R = [[F(wt[3 + 3 * c + r]) for c in range(3)] for r in range(3)]   # transposed
    X, Y, Z = F(v["X"]), F(v["Y"]), F(v["Z"])
    tx = X * R[0][0] + Y * R[0][1] + Z * R[0][2] + t[0]
    ty = X * R[1][0] + Y * R[1][1] + Z * R[1][2] + t[1]
    tz = X * R[2][0] + Y * R[2][1] + Z * R[2][2] + t[2]
    cx, cy, fx, fy = (F(intr[k]) for k in range(4))
    with np.errstate(all="ignore"):
        x = _to_int(float((tx * fx) / tz + cx) + 0.5, floor=True)
        y = _to_int(float(cy - (ty * fy) / tz) + 0.5, floor=True)
        d = max(0, _to_int(float(tz * F(1000.0))))
        d = d & 0xFFFF if _on("d_wraps") else min(d, 65535)
    return x, y, d


def color_transfer(rig, orc, rules=()):
    """Same result as color_ref.color_transfer: (vertices, diagnostics).  rules: names of RULES to compute wrongly."""
    global _RULES
    assert set(rules) <= set(RULES), rules
    _RULES = frozenset(rules)
    try:
        return _color_transfer(rig, orc)
    finally:
        _RULES = frozenset()


def _color_transfer(rig, orc):
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2")
    dc = np.ascontiguousarray(rig.depth_colors)
    S = []
    po = 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        depth = dm[po:po + w * h].reshape(h, w)
        rgb = dc[3 * po:3 * (po + w * h)].reshape(h, w, 3)
        verts, v2p, p2v = orc.create_vertices(depth, rgb, rig.intr[7 * s:7 * s + 7], rig.wt[12 * s:12 * s + 12], rig.bounds, want_maps=True)
        S.append(dict(w=w, h=h, d=[int(v) for v in depth.ravel()], conf=confidence(depth), verts=verts, v2p=list(v2p), p2v=list(p2v),
                      intr=rig.intr[7 * s:7 * s + 7], wt=rig.wt[12 * s:12 * s + 12],
                      col=[(int(v["R"]), int(v["G"]), int(v["B"])) for v in verts]))
        po += w * h
    n = rig.n

    ci = 4 if _on("conf_i_ge_4") else 6 if _on("conf_i_ge_6") else 5
    cj = 4 if _on("conf_j_ge_4") else 6 if _on("conf_j_ge_6") else 5
    thr = {False: 19 if _on("cov_lt_19") else 21 if _on("cov_lt_21") else 20, True: 19 if _on("smp_lt_19") else 21 if _on("smp_lt_21") else 20}
    d1_test = {False: not _on("cov_no_d1_test"), True: _on("smp_d1_test")}
    need = 99 if _on("coverage_gt_99") else 101 if _on("coverage_gt_101") else 100

    def samples(i, j, transform):
        a, b = S[i], S[j]
        out = []
        for v in range(len(b["verts"])):
            x, y, d1 = projection(b["verts"][v], a["intr"], a["wt"])
            if _on("edge_inclusive"):
                x, y = (a["w"] - 1 if x == a["w"] else x), (a["h"] - 1 if y == a["h"] else y)
            if x < 0 or x >= a["w"] or y < 0 or y >= a["h"] or (d1_test[transform] and d1 == 0):
                continue
            q = x + y * a["w"]
            if a["conf"][q] < ci or b["conf"][b["v2p"][v]] < cj:
                continue
            d2 = a["d"][q]
            if d2 > 0 and abs(d1 - d2) < thr[transform]:
                if transform and a["p2v"][q] < 0:
                    continue
                out.append((a["p2v"][q], v))
        return out

    cov = [[0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            cov[i][j] = cov[j][i] = len(samples(i, j, False))
    assigned = [False] * n
    pairs = []
    while True:
        best, b1, b2 = 0, 0, 0
        for i in range(n):
            for j in range(n):
                if i != j and not assigned[j] and assigned[i] and (cov[i][j] > best or (_on("first_branch_last_tie") and cov[i][j] == best > 0)):
                    best, b1, b2 = cov[i][j], i, j
        if best == 0 or (_on("first_branch_falls_through") and best <= need):
            best = 0
            for i in range(n):
                for j in range(i + 1, n):
                    if (cov[i][j] > best or (_on("second_branch_last_tie") and cov[i][j] == best > 0)) and not assigned[i] and not assigned[j]:
                        best, b1, b2 = cov[i][j], i, j
        if best <= need:
            break
        if _on("pair_sorted"):
            b1, b2 = min(b1, b2), max(b1, b2)
        assigned[b1] = assigned[b2] = True
        if _on("bit_31_lost") and n == 32:
            assigned[31] = False
        if len(pairs) >= max(n - 1, 1):   # (only a mutant gets here: every true pair assigns a new map)
            break
        pairs.append((b1, b2))
    xfs = []
    for i, j in pairs:
        sm = samples(i, j, True)
        ne = len(sm)
        if ne == 0:
            xfs.append([0.0] * 6 + [0.0 if _on("empty_scale_0") else 1.0] * 3)
            continue
        src = [S[i]["col"][p] for p, _ in sm]
        dst = [S[j]["col"][v] for _, v in sm]
        m1 = [sum(c[k] for c in src) / float(ne) for k in range(3)]
        m2 = [sum(c[k] for c in dst) / float(ne) for k in range(3)]
        s1, s2 = [0.0] * 3, [0.0] * 3
        for e in range(ne - ne % 8 if _on("fold_tail_dropped") else ne):
            for k in range(3):
                s1[k] += abs(src[e][k] - m1[k])
                s2[k] += abs(dst[e][k] - m2[k])
        s1 = [s / ne + 1e-15 for s in s1]
        s2 = [s / ne + 1e-15 for s in s2]
        xfs.append(m1 + m2 + [s1[k] / s2[k] for k in range(3)])
    out = [s["verts"].copy() for s in S]
    for (i, j), xf in zip(pairs, xfs):
        for v, c in enumerate(S[j]["col"]):
            nc = [min(255, max(0, _to_int((c[k] - xf[3 + k]) * xf[6 + k] + xf[k]))) for k in range(3)]
            out[j][v]["R"], out[j][v]["G"], out[j][v]["B"] = nc
    conf = np.concatenate([np.array(s["conf"], dtype=np.uint8) for s in S])
    return np.concatenate(out), {"confidence": conf, "coverage": np.array(cov), "pairs": pairs, "transforms": np.array(xfs).reshape(-1, 9)}
