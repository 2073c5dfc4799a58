"""A second restatement of the colour transfer in plain Python loops, written after the reference's own control flow (frontier lists,
per-vertex loops), to cross-check tests/color_ref.py on small rigs.  TEST INFRASTRUCTURE ONLY; slow by design.
Float32 arithmetic goes through numpy float32 scalars (one rounding per operation, as the reference's /fp:precise build)."""
import math

import numpy as np

F = np.float32


def _to_int(v):
    """(int) of a Python float (double) on x64."""
    if math.isnan(v) or not (-2147483649.0 < v < 2147483648.0):
        return -2 ** 31
    return int(v)   # truncates toward zero


def confidence(depth):
    h, w = depth.shape
    dm = [int(v) for v in depth.ravel()]
    conf = [20] * (w * h)
    shift_x = [-1, 0, 1, -1, 1, -1, 0, 1]
    shift_y = [-1, -1, -1, 0, 0, 1, 1, 1]
    pos = []
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            p = y * w + x
            if dm[p] == 0:
                conf[p] = 0
                continue
            for s in range(8):
                q = x + shift_x[s] + (y + shift_x[s]) * w   # sic: shift_x in the row offset
                if abs(dm[p] - dm[q]) > 20 or dm[q] == 0:
                    pos.append((x, y))
                    conf[p] = 1
                    break
    max_et = 1
    while pos and max_et != 20:
        new = []
        for x, y in pos:
            d = dm[x + y * w]
            for s in range(8):
                nx, ny = x + shift_x[s], y + shift_y[s]
                if nx <= 0 or ny <= 0 or nx >= w or ny >= h:
                    continue
                q = nx + ny * w
                if abs(d - dm[q]) < 20 and conf[q] == 20 and dm[q] != 0:
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
        x = _to_int(float((tx * fx) / tz + cx) + 0.5)
        y = _to_int(float(cy - (ty * fy) / tz) + 0.5)
        d = min(max(0, _to_int(float(tz * F(1000.0)))), 65535)
    return x, y, d


def color_transfer(rig, orc):
    """Same result as color_ref.color_transfer: (vertices, diagnostics)."""
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

    def samples(i, j, transform):
        a, b = S[i], S[j]
        out = []
        for v in range(len(b["verts"])):
            x, y, d1 = projection(b["verts"][v], a["intr"], a["wt"])
            if x < 0 or x >= a["w"] or y < 0 or y >= a["h"] or (not transform and d1 == 0):
                continue
            q = x + y * a["w"]
            if a["conf"][q] < 5 or b["conf"][b["v2p"][v]] < 5:
                continue
            d2 = a["d"][q]
            if d2 > 0 and abs(d1 - d2) < 20:
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
                if i != j and not assigned[j] and assigned[i] and cov[i][j] > best:
                    best, b1, b2 = cov[i][j], i, j
        if best == 0:
            for i in range(n):
                for j in range(i + 1, n):
                    if cov[i][j] > best and not assigned[i] and not assigned[j]:
                        best, b1, b2 = cov[i][j], i, j
        if best <= 100:
            break
        assigned[b1] = assigned[b2] = True
        pairs.append((b1, b2))
    xfs = []
    for i, j in pairs:
        sm = samples(i, j, True)
        ne = len(sm)
        if ne == 0:
            xfs.append([0.0] * 6 + [1.0] * 3)
            continue
        src = [S[i]["col"][p] for p, _ in sm]
        dst = [S[j]["col"][v] for _, v in sm]
        m1 = [sum(c[k] for c in src) / float(ne) for k in range(3)]
        m2 = [sum(c[k] for c in dst) / float(ne) for k in range(3)]
        s1, s2 = [0.0] * 3, [0.0] * 3
        for e in range(ne):
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
