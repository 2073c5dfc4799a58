"""A second restatement of the render stage (tests/render_ref.py is the numpy one; DESIGN.md section 14 the text) in plain Python: one
view of one tick, a loop per vertex, per triangle and per pixel of its box.  TEST INFRASTRUCTURE ONLY; slow by design.  The 28.4
arithmetic is in Python ints, every float step is one operation on numpy float32 scalars (one rounding each), in the order of
drawTriangle (src/NativeUtils/depthprocessing.cpp:598-706) and pointProjection (:735-747); nothing here calls color_ref.project,
merge_ref.triangle_setup or render_ref.walk.

render(..., rules=...) computes the neighbouring WRONG rule instead of the true one at one decision (RULES: name -> what it does): the
mutants tests/test_render_boundary_ref.py uses to show that a case decides an output.  Without rules nothing changes."""
import math

import numpy as np

F = np.float32
INT_MIN = -2 ** 31

RULES = {
    # projection and drawability
    "project_floor": "x and y are rounded down after the + 0.5, not truncated toward zero",
    "project_rint": "x and y are rint (half to even) of the position, without the + 0.5",
    "x_le_w": "x == w counts as drawable", "y_le_h": "y == h counts as drawable",
    "d0_drawable": "a vertex of d == 0 counts as drawable",
    "d_wraps": "d is cut to its low 16 bits, not clamped at 65535", "d_abs": "d is |d|, not clamped at 0",
    # which triangles are drawn
    "any_vertex": "a triangle is dropped only when all three vertices are undrawable",
    "index_clamped": "an out-of-range index is clamped to the tick's vertices, the triangle drawn",
    "den0_drawn": "a triangle of den == 0 goes through the loops (every val is 0: only its box shows, in `boxes`)",
    "both_windings": "a triangle of the other winding is drawn with corners 2 and 3 swapped",
    # fill rule and box
    "edge_gt": "a pixel is covered when the three edge values are > 0",
    "box_closed": "the box is closed: maxx + 1, maxy + 1",
    # depth value
    "val_round": "val is rounded to nearest, not truncated", "w3_grouped": "w3 = 1 - (w1 + w2)",
    "recip_den": "w1 and w2 are multiplied by 1 / den", "val_fma": "fd1 w1 + fd2 w2 with one rounding (a fused multiply-add)",
    # z-buffer
    "val0_drawn": "candidates of val == 0 take part", "tie_higher": "the higher triangle index wins a tie on val",
    "last_wins": "no depth test: the last triangle drawn owns the pixel",
    "min_vertex_d": "the triangle's smallest vertex d is compared, not the pixel's val",
    # colour
    "color_rint": "rint (half to even) of the sum, not + 0.5 and truncation", "color_sum_order": "c1 w1 + (c2 w2 + c3 w3)",
    "color_fma": "c1 w1 + c2 w2 with one rounding (a fused multiply-add)",
    "color_bgr": "R and B swapped", "color_flat": "the colour of corner 1 alone",
    # points mode
    "points_tie_higher": "the higher vertex index wins a tie on d", "points_last_wins": "no depth test: the last vertex owns the pixel",
    "points_clamped": "a vertex off the image (d != 0) is drawn at the nearest pixel",
}
# Left out, with what was searched:
#   "the C++ of the fill convention is left out": no input tells it from the right rule.  Projected corners are integers, so in 28.4 every
#       C, every DX * (16 y) and every DY * (16 x) is a multiple of 256 and so is each edge value before the ++; e >= 0 and e + 1 >= 0 are then
#       the same test.  (It follows that a pixel on an edge belongs to both sides; what keeps a shared horizontal or vertical edge single is
#       the half-open box.  The case shared_edges holds that.)
#   "colour without the clamp to [0, 255]": it has no witness.  v = ((c1 w1 + c2 w2) + c3 w3) + 0.5 leaves (-1, 256) only if the weights'
#       sum leaves 1 by more than 0.5 / 255 or a weight falls below -0.5 / 255.  Over every triangle with corners on a 7 x 7 grid (117649
#       corner triples, 268800 covered pixels, through render_ref.walk) the sum stays within 6e-8 of 1 and no weight is below -6e-8; with 0
#       and 255 at the corners in all eight ways v stays in [0.49998, 255.50003], and the truncation of that is already a byte.  (With
#       d = 65535 at the corners val is 65534 or 65535 there: a val that wraps past 16 bits has no witness either.)
#   "the last drawn wins (no index in the key)" as a rule of its own beside tie_higher: in a sequential restatement a key without the
#       index IS "the later candidate replaces an equal one", which is tie_higher; last_wins here is the painter's form (no depth test).


def _to_int(v, floor=False):
    """(int) of a Python float (double) on x64: cvttsd2si."""
    if math.isnan(v) or not (-2147483649.0 < v < 2147483648.0):
        return INT_MIN
    return math.floor(v) if floor else int(v)      # int() truncates toward zero


def _u16(v, nearest=False):
    """(unsigned short) of a float32 on x64: cvttss2si (INT_MIN out of int32), then the low 16 bits."""
    v = float(v)
    if math.isnan(v) or not (-2147483648.0 <= v < 2147483648.0):
        return INT_MIN & 0xFFFF
    return (math.floor(v + 0.5) if nearest else int(v)) & 0xFFFF


def _pixel_coordinate(pos32, on):
    """The integer pixel coordinate of a float32 image position."""
    p = float(pos32)
    if "project_rint" in on:
        return INT_MIN if math.isnan(p) or math.isinf(p) or not (-2147483649.0 < p < 2147483648.0) else int(round(p))   # half to even
    return _to_int(p + 0.5, floor="project_floor" in on)      # the + 0.5 is a double add


def project(X, Y, Z, intr, wt, on=frozenset()):
    """pointProjection with the inverted pose (R -> R^T, t -> -t; rotate, then add).  Returns Python ints (x, y, d)."""
    t = [-F(wt[0]), -F(wt[1]), -F(wt[2])]
    R = [[F(wt[3 + 3 * c + r]) for c in range(3)] for r in range(3)]      # transposed
    X, Y, Z = F(X), F(Y), F(Z)
    cx, cy, fx, fy = (F(intr[k]) for k in range(4))
    with np.errstate(all="ignore"):
        tx = (X * R[0][0] + Y * R[0][1] + Z * R[0][2]) + t[0]
        ty = (X * R[1][0] + Y * R[1][1] + Z * R[1][2]) + t[1]
        tz = (X * R[2][0] + Y * R[2][1] + Z * R[2][2]) + t[2]
        x = _pixel_coordinate((tx * fx) / tz + cx, on)
        y = _pixel_coordinate(cy - (ty * fy) / tz, on)
        d = _to_int(float(tz * F(1000.0)))
    d = abs(d) if "d_abs" in on else max(d, 0)
    return x, y, (d & 0xFFFF if "d_wraps" in on else min(d, 65535))


def _byte(v, on):
    """A colour channel from the float32 sum (the + 0.5 not yet added)."""
    if "color_rint" in on:
        i = int(np.rint(v))
    else:
        i = int(v + F(0.5))
    return min(max(i, 0), 255)


def render(verts, tris, intr7, wt12, w, h, rules=(), terms=None):
    """One view of one tick, as render_ref.render: (depth u16 (h, w), rgb u8 (h, w, 3), {"drawn", "pixels", "boxes"}).  rules: names of
    RULES to compute wrongly.  terms: a list that receives one record of the intermediate values."""
    on = frozenset(rules)
    assert on <= set(RULES), sorted(on - set(RULES))
    assert 1 <= w <= 1024 and 1 <= h <= 1024
    nv = len(verts)
    P = []
    for g in range(nv):
        x, y, d = project(verts["X"][g], verts["Y"][g], verts["Z"][g], intr7, wt12, on)
        ok = 0 <= x and (x <= w if "x_le_w" in on else x < w) and 0 <= y and (y <= h if "y_le_h" in on else y < h)
        ok = ok and (d != 0 or "d0_drawable" in on)
        P.append((x, y, d, ok))
    col = [(int(verts["R"][g]), int(verts["G"][g]), int(verts["B"][g])) for g in range(nv)]
    best = {}      # pixel -> what won it
    rec = {"x": [p[0] for p in P], "y": [p[1] for p in P], "d": [p[2] for p in P], "ok": [bool(p[3]) for p in P], "cand": []}
    drawn, boxes = 0, []

    def inside(px, py):      # the wrong rules alone can reach outside the image; such a pixel does not exist
        return 0 <= px < w and 0 <= py < h

    if tris is None:
        for g in range(nv):
            x, y, d, ok = P[g]
            if not ok and "points_clamped" in on and d != 0:
                x, y, ok = min(max(x, 0), w - 1), min(max(y, 0), h - 1), True
            if not ok:
                continue
            drawn += 1
            if not inside(x, y):
                continue
            b = best.get((x, y))
            if b is None or "points_last_wins" in on or d < b[0] or (d == b[0] and "points_tie_higher" in on):
                best[(x, y)] = (d, g)
        out = {p: (d, col[g]) for p, (d, g) in best.items()}
    else:
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        for t in range(len(tris)):
            i1, i2, i3 = (int(v) for v in tris[t])
            if not all(0 <= i < nv for i in (i1, i2, i3)):
                if "index_clamped" not in on or nv == 0:
                    continue
                i1, i2, i3 = (min(max(i, 0), nv - 1) for i in (i1, i2, i3))
            oks = [P[i][3] for i in (i1, i2, i3)]
            if not (any(oks) if "any_vertex" in on else all(oks)):
                continue
            drawn += 1
            (x1, y1, d1, _), (x2, y2, d2, _), (x3, y3, d3, _) = P[i1], P[i2], P[i3]
            den = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3)                                      # :656, :660
            if den > 0 and "both_windings" in on:      # den < 0 is the winding the half-space test draws
                i2, i3, x2, y2, d2, x3, y3, d3 = i3, i2, x3, y3, d3, x2, y2, d2
                den = -den
            X1, X2, X3, Y1, Y2, Y3 = 16 * x1, 16 * x2, 16 * x3, 16 * y1, 16 * y2, 16 * y3          # 28.4 of integer positions (:602-609)
            DX12, DX23, DX31, DY12, DY23, DY31 = X1 - X2, X2 - X3, X3 - X1, Y1 - Y2, Y2 - Y3, Y3 - Y1
            minx, maxx = (min(X1, X2, X3) + 0xF) >> 4, (max(X1, X2, X3) + 0xF) >> 4                  # :629-632, half-open
            miny, maxy = (min(Y1, Y2, Y3) + 0xF) >> 4, (max(Y1, Y2, Y3) + 0xF) >> 4
            if "box_closed" in on:
                maxx, maxy = maxx + 1, maxy + 1
            C1, C2, C3 = DY12 * X1 - DX12 * Y1, DY23 * X2 - DX23 * Y2, DY31 * X3 - DX31 * Y3        # :639-641
            C1 += DY12 < 0 or (DY12 == 0 and DX12 > 0)                                               # the fill convention (:644-646)
            C2 += DY23 < 0 or (DY23 == 0 and DX23 > 0)
            C3 += DY31 < 0 or (DY31 == 0 and DX31 > 0)
            if den == 0 and "den0_drawn" not in on:                                                  # :662-663
                boxes.append(0)
                continue
            boxes.append((maxx - minx) * (maxy - miny))
            fden, y23, x32, y31, x13 = F(den), F(y2 - y3), F(x3 - x2), F(y3 - y1), F(x1 - x3)
            fd1, fd2, fd3 = F(d1), F(d2), F(d3)
            for py in range(max(miny, 0), min(maxy, h)):
                for px in range(max(minx, 0), min(maxx, w)):
                    e1 = C1 + DX12 * (16 * py) - DY12 * (16 * px)                                    # :648-650, :697-703 in closed form
                    e2 = C2 + DX23 * (16 * py) - DY23 * (16 * px)
                    e3 = C3 + DX31 * (16 * py) - DY31 * (16 * px)
                    if not on:
                        assert all(abs(v) < 2 ** 31 for v in (C1, C2, C3, e1, e2, e3, DX12 * 16 * py, DY12 * 16 * px)), "a 28.4 product left int32"
                    if not ((e1 > 0 and e2 > 0 and e3 > 0) if "edge_gt" in on else (e1 >= 0 and e2 >= 0 and e3 >= 0)):
                        continue
                    with np.errstate(all="ignore"):      # (den == 0 only under den0_drawn)
                        dx3, dy3 = F(px - x3), F(py - y3)
                        term21, term22 = x32 * dy3, x13 * dy3                                        # :671-672
                        n1, n2 = y23 * dx3 + term21, y31 * dx3 + term22
                        if "recip_den" in on:
                            r = F(1.0) / fden
                            w1, w2 = n1 * r, n2 * r
                        else:
                            w1, w2 = n1 / fden, n2 / fden                                            # :677-678
                        w3 = F(1.0) - (w1 + w2) if "w3_grouped" in on else (F(1.0) - w1) - w2       # :679
                        if "val_fma" in on:      # the exact product in double, one rounding of the sum
                            s12 = F(float(fd1) * float(w1) + float(fd2 * w2))
                        else:
                            s12 = fd1 * w1 + fd2 * w2
                        val = _u16(s12 + fd3 * w3, nearest="val_round" in on)                       # :682
                    rec["cand"].append((t, px, py, val, w1, w2, w3))
                    if val == 0 and "val0_drawn" not in on:
                        continue
                    cmp = min(d1, d2, d3) if "min_vertex_d" in on else val
                    b = best.get((px, py))
                    if b is None or "last_wins" in on or cmp < b[0] or (cmp == b[0] and "tie_higher" in on):
                        best[(px, py)] = (cmp, t, val, (w1, w2, w3), (i1, i2, i3))
        out, rec["v"] = {}, {}
        for p, (_, t, val, (w1, w2, w3), (i1, i2, i3)) in best.items():
            rgb = []
            for ch in range(3):
                f1, f2, f3 = F(col[i1][ch]), F(col[i2][ch]), F(col[i3][ch])
                with np.errstate(all="ignore"):
                    if "color_flat" in on:
                        v = f1
                    elif "color_sum_order" in on:
                        v = f1 * w1 + (f2 * w2 + f3 * w3)
                    elif "color_fma" in on:      # the exact product in double, one rounding of the sum
                        v = F(float(f1) * float(w1) + float(f2 * w2)) + f3 * w3
                    else:
                        v = (f1 * w1 + f2 * w2) + f3 * w3
                rgb.append(0 if math.isnan(float(v)) else _byte(v, on))
                rec["v"].setdefault(p, []).append(v)
            out[p] = (val, tuple(rgb[::-1] if "color_bgr" in on else rgb))
    depth = np.zeros((h, w), dtype=np.uint16)
    rgb = np.zeros((h, w, 3), dtype=np.uint8)
    for (px, py), (d, c) in out.items():
        depth[py, px] = d
        rgb[py, px] = c
    if terms is not None:
        terms.append(rec)
    return depth, rgb, {"drawn": drawn, "pixels": int((depth != 0).sum()), "boxes": np.array(boxes, dtype=np.int64)}
