"""CPU reference of generateMeshFromDepthMaps' cross-view overlay merge (bgenerate_triangles = true).  TEST INFRASTRUCTURE ONLY.

A line-cited restatement (numpy) of src/NativeUtils/depthprocessing.cpp, on top of tests/color_ref.py (vertices, vertex <-> pixel
maps, confidence maps, pointProjection) and the oracle's triangulation (orc.generate_triangles, pinned to meshGenerator.cpp):

  1. reprojection    mergeVerticesForViews :1241-1248, projectVerticesIntoDepthMap :749-782 (includeAssigned = false: nothing
                     is assigned yet), pointProjection :735-747 with the sensor's own inverted pose
  2. per base b, per overlay o != b in increasing order (:1250-1300), assignDepthMapOverlay :932-1099:
       a. mapDepthMap :840-901 -- o's current maps triangulated (with b's w, h: every sensor has the same size here), o's
          unassigned vertices projected into b (dropped for x < 1, x >= w, y < 1, y >= h, d == 0), every triangle with three
          non-zero depths drawn (drawTriangle :598-706) with the tag (c1 + c2 + c3) / 3.0f
       b. the replace mask :989-1020, c. morphologyErode twice :903-930, d. zero + point_assigned :1026-1032
  3. generateTriangles :1659-1691 on the final maps, formMesh's rebase :1611-1627

The drawTriangle loop's "d == 0 || val < depth_map[x]" (:684) is evaluated in closed form: per pixel the covering triangle of
smallest (val, index) among those after the last covering triangle whose val is 0 (Z); if there is none, depth 0 with Z's tag.
draw_sequential restates the loop literally (tests/test_merge_ref.py checks the two against each other and against the reference's
own drawTriangle through tests/golden/overlay_merge_ref.npz).

Pinned as a whole: tests/golden/export_ref.npz / export_ref_digests.json hold the reference's own
generateMeshFromDepthMaps(bgenerate_triangles = true), alone and after colour transfer, on wall, twins, ring and edge rigs
(tests/golden/make_export_golden.py); tests/test_export_pin.py holds overlay_merge() to them.  tests/golden/merge_boundary_ref.npz
holds the same call on the boundary rigs of tests/merge_boundary_cases.py -- 1 mm depths, unequal intrinsics, zero writers, colliding
reprojections (tests/golden/make_merge_boundary_golden.py); tests/test_merge_boundary_ref.py holds overlay_merge() to it.

Defined where the reference is not: float -> unsigned short is x64's (cvttss2si to int32, INT_MIN for NaN and
out of range, then the low 16 bits); every sensor must have the same size (mixed sizes are not in the export fixtures).

Two keyword arguments serve tests/test_merge_boundary_ref.py (defaults: neither; the restatement is then what it always was):
  trace=   a dict (records are appended to trace[kind]) or a callable trace(kind, record); kinds "reproject" (per sensor), "map" (per
           (base, overlay): the projection and the triangles of mapDepthMap), "draw" (per drawTriangle pass: the triangles, their tags
           and the per-pixel class, CLASSES) and "overlay" (per (base, overlay): the base depth before the mask, the mapped depth and
           tag, the raw and the eroded mask); a record names its place by "s" (sensor) or "b" and "o" (base, overlay);
  rules=   names out of RULES: each flips ONE decision of the restatement (a mutant), so that a test can show that a rig's output
           depends on that decision."""
import numpy as np

from tests import color_ref

DEPTH_THRESHOLD = 20   # :934
CONF_THRESHOLD = 5     # :1007
INT_MIN = -2 ** 31
f32 = np.float32

# the per-pixel classes of a draw (trace kind "draw", key "classes"); Z = the last covering triangle whose val is 0
NEVER, ONE_WRITER, SEVERAL_NONE_ZERO, ZERO_THEN_LATER, SMALLER_DISCARDED, ZERO_ONLY = range(6)
CLASSES = ("never covered", "one writer", "several writers, none zero", "zero writer followed by a later writer",
           "earlier smaller val discarded by a zero writer", "zero writers only")
# ZERO_THEN_LATER:   a writer behind Z decides the pixel (the kernel's t > zmax filter lets it through, zmax must be reset afterwards)
# SMALLER_DISCARDED: as ZERO_THEN_LATER, and a writer before Z had a non-zero val below the winner's (the plain minimum would keep it)
# ZERO_ONLY:         nothing behind Z: depth 0 with Z's tag (the resolve kernel's "key is none" branch)

RULES = {
    "depth_threshold_19": "|base - mapped| < 19 for < 20 (:934)",
    "depth_threshold_21": "|base - mapped| < 21 for < 20 (:934)",
    "conf_threshold_4": "tag > 4 for > 5 (:1007)",
    "conf_threshold_6": "tag > 6 for > 5 (:1007)",
    "zero_writers_ignored": "drawTriangle as the plain minimum of (val, index) (:684 without d == 0)",
    "k_ge_z": "the writers k >= Z compete, not k > Z: Z's own 0 wins",
    "nonzero_minimum": "every writer with a non-zero val competes, those before Z too: the smallest non-zero (val, index)",
    "drop_lt_0": "mapDepthMap drops x < 0 / y < 0 for x < 1 / y < 1 (:867)",
    "drop_gt_wh": "mapDepthMap drops x > w / y > h for x >= w / y >= h (:867)",
    "reproject_d0_test": "a d == 0 test added to projectVerticesIntoDepthMap (:773)",
    "first_vertex_wins": "the first vertex on a pixel keeps it in projectVerticesIntoDepthMap (:768-778)",
    "den0_drawn": "triangles with den == 0 drawn: the NaN / inf weights convert to val 0 (:662)",
    "one_erosion": "morphologyErode once (:1023-1024)",
    "overlays_decreasing": "the overlays of a base visited in decreasing order (:1276-1283)",
    "one_dropped_vertex_drawn": "a triangle with exactly one dropped vertex drawn with that vertex at (0, 0, 0) (:885)",
}

# Mutants that rules= accepts as well, but that no rig can kill through generateMeshFromDepthMaps (tests/merge_boundary_cases.py says why):
# they are not part of the decisiveness table.
UNDECIDED_RULES = {
    "border_cleared": "morphologyErode clears the border rows and columns",
    "assigned_ignored": "mapDepthMap projects assigned vertices too (:860)",
}


def _emit(trace, kind, **record):
    if trace is None:
        return
    if callable(trace):
        trace(kind, record)
    else:
        trace.setdefault(kind, []).append(record)


def _rules(rules):
    rules = frozenset(rules or ())
    assert rules <= set(RULES) | set(UNDECIDED_RULES), sorted(rules - set(RULES) - set(UNDECIDED_RULES))
    return rules


def cvt_u16_x64(v):
    """(unsigned short)v of float32 values as x64 code computes it: cvttss2si (INT_MIN for NaN / out of int32), then the low 16 bits."""
    v = np.asarray(v, dtype=np.float32)
    ok = (v >= f32(-2147483648.0)) & (v < f32(2147483648.0))
    i = np.where(ok, np.trunc(np.where(ok, v, f32(0))).astype(np.int64), INT_MIN)
    return (i & 0xFFFF).astype(np.int64)


def _wrap32(a):
    a = np.asarray(a, dtype=np.int64) & 0xFFFFFFFF
    return np.where(a >= 2 ** 31, a - 2 ** 32, a)


def triangle_setup(x1, y1, d1, x2, y2, d2, x3, y3, d3):
    """Per triangle (int arrays): what drawTriangle (:598-666) derives before its loop.  Returns a dict of int64 / float32 arrays."""
    x1, y1, x2, y2, x3, y3 = (np.asarray(a, dtype=np.int64) for a in (x1, y1, x2, y2, x3, y3))
    X1, X2, X3, Y1, Y2, Y3 = 16 * x1, 16 * x2, 16 * x3, 16 * y1, 16 * y2, 16 * y3      # iround(16.0f * v) of integers (:602-609)
    DX12, DX23, DX31, DY12, DY23, DY31 = X1 - X2, X2 - X3, X3 - X1, Y1 - Y2, Y2 - Y3, Y3 - Y1
    s = dict(minx=(np.minimum(np.minimum(X1, X2), X3) + 0xF) >> 4, maxx=(np.maximum(np.maximum(X1, X2), X3) + 0xF) >> 4,   # :629-632
             miny=(np.minimum(np.minimum(Y1, Y2), Y3) + 0xF) >> 4, maxy=(np.maximum(np.maximum(Y1, Y2), Y3) + 0xF) >> 4)
    C = []
    for DY, DX, X, Y in ((DY12, DX12, X1, Y1), (DY23, DX23, X2, Y2), (DY31, DX31, X3, Y3)):
        c = DY * X - DX * Y                                                              # :639-641
        c = c + ((DY < 0) | ((DY == 0) & (DX > 0)))                                      # fill convention :644-646
        C.append((c, DX, DY))
    s["C"] = C
    s["den"] = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3)                             # :656, :660 (int; den1 == den2)
    s["y23"], s["x32"] = (y2 - y3).astype(f32), (x3 - x2).astype(f32)
    s["y31"], s["x13"] = (y3 - y1).astype(f32), (x1 - x3).astype(f32)
    s["x3"], s["y3"] = x3, y3
    s["fd"] = [np.asarray(d, dtype=np.int64).astype(f32) for d in (d1, d2, d3)]
    return s


def triangle_pixels(s, rules=frozenset()):
    """Every (triangle, pixel) the loops of :668-705 visit that passes the edge test, with its val.  Returns (k, x, y, val)."""
    bw = np.maximum(s["maxx"] - s["minx"], 0)
    bh = np.maximum(s["maxy"] - s["miny"], 0)
    cnt = np.where((s["den"] != 0) | ("den0_drawn" in rules), bw * bh, 0)                # den == 0: no pixel (:662-663)
    k = np.repeat(np.arange(len(cnt)), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    bwk = bw[k]
    px = s["minx"][k] + j % np.maximum(bwk, 1)
    py = s["miny"][k] + j // np.maximum(bwk, 1)
    inside = np.ones(len(k), dtype=bool)
    for c, DX, DY in s["C"]:
        # CX after the row / column steps of :648-650, :697-703 (int32 arithmetic)
        inside &= _wrap32(c[k] + DX[k] * (16 * py) - DY[k] * (16 * px)) >= 0
    k, px, py = k[inside], px[inside], py[inside]
    fden = s["den"][k].astype(f32)
    dx3, dy3 = (px - s["x3"][k]).astype(f32), (py - s["y3"][k]).astype(f32)
    term21, term22 = s["x32"][k] * dy3, s["x13"][k] * dy3                              # :671-672
    with np.errstate(all="ignore"):                                                     # (den == 0 only under the den0_drawn rule)
        w1 = (s["y23"][k] * dx3 + term21) / fden                                        # :677
        w2 = (s["y31"][k] * dx3 + term22) / fden                                        # :678
        w3 = f32(1.0) - w1 - w2                                                         # :679
        fd1, fd2, fd3 = (f[k] for f in s["fd"])
        val = cvt_u16_x64(fd1 * w1 + fd2 * w2 + fd3 * w3)                               # :682
    return k, px, py, val


def pixel_classes(k, p, val, npix):
    """The class (CLASSES) of every pixel of a draw from its writers: triangle k writes val at pixel p."""
    big = np.iinfo(np.int64).max
    cover = np.bincount(p, minlength=npix)
    z = np.full(npix, -1, dtype=np.int64)
    np.maximum.at(z, p[val == 0], k[val == 0])
    after = k > z[p]
    win = np.full(npix, big, dtype=np.int64)
    np.minimum.at(win, p[after], val[after])
    before = (k < z[p]) & (val != 0)
    low = np.full(npix, big, dtype=np.int64)
    np.minimum.at(low, p[before], val[before])
    cls = np.select([cover == 0, (z >= 0) & (win == big), (z >= 0) & (low < win), z >= 0, cover == 1],
                    [NEVER, ZERO_ONLY, SMALLER_DISCARDED, ZERO_THEN_LATER, ONE_WRITER], SEVERAL_NONE_ZERO)
    return cls


def draw(tris, tags, w, h, trace=None, rules=None, **where):
    """drawTriangle (:598-706) of tris (m, 9) int {x1,y1,d1,x2,y2,d2,x3,y3,d3}, in order, into a zeroed (h, w) map, tags int (m,):
    the closed form of the sequential loop.  Returns (depth u16 (h, w), tag u16 (h, w)).  `where` goes into the trace record."""
    rules = _rules(rules)
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 9)
    tags = np.asarray(tags, dtype=np.int64)
    depth = np.zeros(h * w, dtype=np.int64)
    tag = np.zeros(h * w, dtype=np.int64)
    if len(tris) == 0:
        _emit(trace, "draw", tris=tris, tags=tags, w=w, h=h, classes=np.zeros((h, w), dtype=np.int64), **where)
        return depth.reshape(h, w).astype(np.uint16), tag.reshape(h, w).astype(np.uint16)
    k, px, py, val = triangle_pixels(triangle_setup(*tris.T), rules)
    p = py * w + px
    if trace is not None:
        _emit(trace, "draw", tris=tris, tags=tags, w=w, h=h, classes=pixel_classes(k, p, val, h * w).reshape(h, w), **where)
    z = np.full(h * w, -1, dtype=np.int64)
    zero = (val == 0) & ("zero_writers_ignored" not in rules)
    np.maximum.at(z, p[zero], k[zero])                                                  # the last val-0 writer
    after = (k >= z[p]) if "k_ge_z" in rules else (val != 0) if "nonzero_minimum" in rules else (k > z[p])
    key = np.full(h * w, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(key, p[after], (val[after] << 32) | k[after])                         # smallest (val, index) behind it
    won = key != np.iinfo(np.int64).max
    depth[won] = key[won] >> 32
    tag[won] = tags[key[won] & 0xFFFFFFFF]
    only_zero = ~won & (z >= 0)
    tag[only_zero] = tags[z[only_zero]]
    return depth.reshape(h, w).astype(np.uint16), tag.reshape(h, w).astype(np.uint16)


def draw_sequential(tris, tags, w, h, depth=None, tag=None):
    """drawTriangle (:598-706) as the reference loops, triangle by triangle and pixel by pixel (plain Python, small inputs)."""
    depth = np.zeros((h, w), dtype=np.int64) if depth is None else depth.astype(np.int64)
    tag = np.zeros((h, w), dtype=np.int64) if tag is None else tag.astype(np.int64)
    for t, tg in zip(np.asarray(tris, dtype=np.int64).reshape(-1, 9), tags):
        k, px, py, val = triangle_pixels(triangle_setup(*[t[i:i + 1] for i in range(9)]))
        order = np.lexsort((px, py))                                                    # row by row, left to right (:668-705)
        for x, y, v in zip(px[order], py[order], val[order]):
            d = depth[y, x]
            if d == 0 or v < d:                                                         # :684
                depth[y, x] = v
                tag[y, x] = tg
    return depth.astype(np.uint16), tag.astype(np.uint16)


def erode(mask):
    """morphologyErode (:903-930) on an (h, w) bool mask: interior pixels with a cleared 8-neighbour are cleared; the border stays."""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    out = m.copy()
    if h < 3 or w < 3:
        return out
    inner = m[1:h - 1, 1:w - 1].copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                inner &= m[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    out[1:h - 1, 1:w - 1] = inner
    return out


def erode_loop(mask):
    """morphologyErode restated as the reference loops (plain Python)."""
    m = [[bool(v) for v in row] for row in np.asarray(mask)]
    h, w = len(m), len(m[0]) if m else 0
    sx = (-1, 0, 1, -1, 1, -1, 0, 1)
    sy = (-1, -1, -1, 0, 0, 1, 1, 1)
    out = [row[:] for row in m]
    for j in range(1, h - 1):
        for i in range(1, w - 1):
            if not m[j][i]:
                continue
            for s in range(8):
                if not m[j + sy[s]][i + sx[s]]:
                    out[j][i] = False
                    break
    return np.array(out, dtype=bool).reshape(h, w)


class _State:
    def __init__(self, sensor):
        self.s = sensor
        self.depth = np.zeros(sensor.h * sensor.w, dtype=np.int64)      # depth_map after the reprojection
        self.d2v = np.full(sensor.h * sensor.w, -1, dtype=np.int64)     # depth_to_vertices_map
        self.assigned = np.zeros(len(sensor.verts), dtype=bool)          # point_assigned


def _sensors(rig, orc):
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2")
    dc = np.ascontiguousarray(rig.depth_colors)
    out, po = [], 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        out.append(color_ref.Sensor(dm[po:po + w * h].reshape(h, w), dc[3 * po:3 * (po + w * h)].reshape(h, w, 3), rig.intr[7 * s:7 * s + 7],
                                    rig.wt[12 * s:12 * s + 12], rig.bounds, orc))
        po += w * h
    return out


def reproject(st, trace=None, rules=None, **where):
    """projectVerticesIntoDepthMap (:749-782) with the sensor's own inverted pose, includeAssigned = false, nothing assigned yet."""
    rules = _rules(rules)
    s = st.s
    x, y, d = color_ref.project(s.verts["X"], s.verts["Y"], s.verts["Z"], s.intr, s.wt)
    inb = (x >= 0) & (x < s.w) & (y >= 0) & (y < s.h)                                  # :773-774 (no d == 0 test)
    if "reproject_d0_test" in rules:
        inb &= d != 0
    pix = (y * s.w + x)[inb]
    idx = np.flatnonzero(inb)
    if "first_vertex_wins" in rules:
        first = np.full(len(st.d2v), len(x), dtype=np.int64)
        np.minimum.at(first, pix, idx)
        st.d2v[first < len(x)] = first[first < len(x)]
    else:
        np.maximum.at(st.d2v, pix, idx)                                                 # the last vertex wins (:768-778)
    hit = st.d2v >= 0
    st.depth[hit] = d[st.d2v[hit]]
    _emit(trace, "reproject", x=x, y=y, d=d, inb=inb, v2p=s.v2p, w=s.w, h=s.h, **where)


def map_depth_map(ov, base, orc, trace=None, rules=None, **where):
    """mapDepthMap (:840-901) of overlay state `ov` into the camera of `base`.  Returns (mapped depth, tag) (h, w)."""
    rules = _rules(rules)
    s, b = ov.s, base.s
    w, h = b.w, b.h
    tris = orc.generate_triangles(ov.depth.reshape(h, w).astype(np.uint16), ov.d2v.astype(np.int32))   # :844-845 (b's w, h)
    x, y, d = color_ref.project(s.verts["X"], s.verts["Y"], s.verts["Z"], b.intr, b.wt)                   # :851 inv, :866
    low = 0 if "drop_lt_0" in rules else 1
    out = ((x > w) | (y > h)) if "drop_gt_wh" in rules else ((x >= w) | (y >= h))
    free = np.ones_like(ov.assigned) if "assigned_ignored" in rules else ~ov.assigned
    ok = free & ~((x < low) | (y < low) | out | (d == 0))                                               # :860-861, :867-868
    ds, xs, ys = np.where(ok, d, 0), np.where(ok, x, 0), np.where(ok, y, 0)
    conf = np.where(ok, s.conf[s.v2p].astype(np.int64), 0)                                             # :874
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    i1, i2, i3 = tris[:, 0], tris[:, 1], tris[:, 2]
    dropped = (ds[i1] == 0).astype(np.int64) + (ds[i2] == 0) + (ds[i3] == 0)
    keep = dropped <= (1 if "one_dropped_vertex_drawn" in rules else 0)                 # :885-886
    _emit(trace, "map", x=x, y=y, d=d, assigned=ov.assigned.copy(), ok=ok, tris=tris, dropped=dropped, w=w, h=h, **where)
    i1, i2, i3 = i1[keep], i2[keep], i3[keep]
    tags = cvt_u16_x64((conf[i1] + conf[i2] + conf[i3]).astype(f32) / f32(3.0))         # :889
    t9 = np.stack([xs[i1], ys[i1], ds[i1], xs[i2], ys[i2], ds[i2], xs[i3], ys[i3], ds[i3]], axis=1)
    return draw(t9, tags, w, h, trace, rules, **where)


def assign_overlay(base, ov, orc, trace=None, rules=None, **where):
    """assignDepthMapOverlay (:932-1099) of overlay `ov` onto `base`: mask, two erosions, zero + assign."""
    rules = _rules(rules)
    mapped, tag = map_depth_map(ov, base, orc, trace, rules, **where)
    mapped, tag = mapped.ravel().astype(np.int64), tag.ravel().astype(np.int64)
    b = base.s
    dthr = 19 if "depth_threshold_19" in rules else 21 if "depth_threshold_21" in rules else DEPTH_THRESHOLD
    cthr = 4 if "conf_threshold_4" in rules else 6 if "conf_threshold_6" in rules else CONF_THRESHOLD
    raw = (base.depth != 0) & (np.abs(base.depth - mapped) < dthr) & (tag > cthr)                       # :989-1020
    mask = raw.reshape(b.h, b.w)
    for _ in range(1 if "one_erosion" in rules else 2):                                                 # :1023-1024
        mask = erode(mask)
        if "border_cleared" in rules:
            mask[[0, -1], :] = False
            mask[:, [0, -1]] = False
    mask = mask.ravel()
    _emit(trace, "overlay", base_depth=base.depth.copy(), mapped=mapped, tag=tag, mask_raw=raw, mask_eroded=mask.copy(), w=b.w, h=b.h, **where)
    base.depth[mask] = 0                                                                               # :1026-1032
    base.assigned[base.d2v[mask]] = True


def overlay_merge(rig, orc, trace=None, rules=None):
    """generateMeshFromDepthMaps(..., bgenerate_triangles = true)'s triangles for a synth.Rig of equal-sized sensors.
    Returns (triangles int32 (m, 3), {"reprojected": u16 per tick pixel, "merged": u16 per tick pixel, "assigned": u8 per vertex,
    "offsets": vertex offsets [n+1]})."""
    sensors = _sensors(rig, orc)
    assert all(s.w == sensors[0].w and s.h == sensors[0].h for s in sensors), "the merge needs equal sensor sizes"
    rules = _rules(rules)
    st = [_State(s) for s in sensors]
    for k, x in enumerate(st):
        reproject(x, trace, rules, s=k)
    reprojected = np.concatenate([x.depth for x in st]).astype(np.uint16)
    n = len(st)
    for b in range(n):                                                                   # :1250
        for o in (range(n - 1, -1, -1) if "overlays_decreasing" in rules else range(n)):   # :1276-1283
            if o != b:
                assign_overlay(st[b], st[o], orc, trace, rules, b=b, o=o)
    off = np.concatenate([[0], np.cumsum([len(s.verts) for s in sensors])]).astype(np.int64)
    tris = [orc.generate_triangles(x.depth.reshape(x.s.h, x.s.w).astype(np.uint16), x.d2v.astype(np.int32), int(off[k]))
            for k, x in enumerate(st)]                                                   # :1659-1691, formMesh :1611-1627
    tris = np.concatenate(tris).astype(np.int32) if tris else np.zeros((0, 3), np.int32)
    return tris, {"reprojected": reprojected, "merged": np.concatenate([x.depth for x in st]).astype(np.uint16),
                  "assigned": np.concatenate([x.assigned for x in st]).astype(np.uint8), "offsets": off}
