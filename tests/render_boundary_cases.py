"""Hand-made cases for the render stage (livescan3d_amd/csrc/render.hip, livescan3d_amd/csrc/raster.hip; the definition: DESIGN.md
section 14, restated twice in tests/render_ref.py and tests/render_ref_py.py).  Test infrastructure.  tests/test_render_boundary_ref.py holds every case to its
witness on the definition alone -- what the case is named for is reached -- and to the mutants of render_ref_py.RULES it is listed to
kill; tests/test_render_boundary_gpu.py runs the cases through lsnFusionRenderViews.

A case is one or more ticks of (vertices, triangles or None), its views (7 + 12 floats each, w, h) and a mode.  Unless it says otherwise
a case is drawn into 32 x 24 pixels from two views with the intrinsics (cx, cy, f) = (16, 12, 32): the identity pose and POSE_A, a
camera turned about two axes and moved.  `view` names the view the witness reads: a case made for the identity shows its picture in
view 0, a "posed" twin (the same camera-frame vertices carried into the world through POSE_A) shows the same integer picture in view 1,
with the witness and the kills of its identity case.  Every case is compared in both views, but the other view of a case is mostly an
empty image (its vertices lie off that camera's image): what reaches a rule through a pose that is not the identity are the posed twins
(one in every group of the small cases), waves, scratch's turned view and views16.

A mutant counts as killed when anything the stage reports differs: the image or the counts.  Three kills are by a count alone and say so
where the case is built: den0_drawn (every val of a den == 0 triangle is 0, so only its box shows: `boxes` here, `large` on the GPU) and,
in points mode, x_le_w / y_le_h (a vertex on x == w or y == h has no pixel: only `drawn` counts it; proj_corners kills both in the image).

  proj_points, proj_corners, proj_corners_z, proj_posed
                                           vertices at u, v around -1.5 .. -0.4 and w - 1.6 .. w - 0.4, on k + 0.5, Z behind, at and
                                           far from the camera, NaN and inf; as points and as corners of triangles
  vertex_out, vertex_out_only, vertex_out_posed, index_out
                                           triangles with one, two, three undrawable corners (off the image, behind the camera,
                                           d = 0) beside whole ones; indices out of range
  winding, winding_posed, mirror_only, degenerate, one_pixel, thin
                                           a triangle and its mirror; den == 0 three ways; boxes of 1 x 1, 1 x n, n x 1
  shared_edges, shared_edges_posed, fan8   five edge directions shared by two triangles; eight triangles around one pixel
  val_d1, val_d12, val_near_far, val_near_far_posed, val_max, val_round, val_fused, w3_order, den_recip
                                           val 0 and 1 from vertices at 1 mm, alone and in front of a far surface; 65534 / 65535;
                                           triangles (found by search) on which one rounding of the value decides a byte
  tie2_ab, tie2_ba, tie3, zbuffer, points_tie, points_posed
                                           different triangles with one val on a common pixel, in every order; a triangle whose nearest
                                           corner is nearer but whose pixel is farther; three vertices on one pixel, d = 7, 5, 5
  color_half, color_half_posed, color_channels, color_extremes, color_order, color_fused
                                           colour sums on k + 0.5, a rounding below and above (found by search); distinct channels;
                                           0 and 255 beside a negative weight; the sum order and a fused product deciding a byte
  boxes_together, boxes_posed, boxes_apart boxes of 15, 16 and 17 pixels around SMALL_BOX
  waves                                    64 x 48: 240 listed triangles against rv_large_kernel's 96 waves
  scratch, scratch_reverse, views16        views of many, none and few listed triangles in one call, an empty tick, junk behind the
                                           counts; 16 views of 8 x 6
  raster_two_pass                          a 512 x 257 plan filled with 263168 triangles: the raster grid's second pass
  budget_1024                              1024 x 1024 covered corner to corner, and a sliver along its diagonal"""
import functools
import itertools

import numpy as np

from tests import render_ref

INT_MIN = -2 ** 31
W, H = 32, 24
INTR = render_ref.intrinsics(W, H)
IDENTITY = render_ref.IDENTITY
SMALL_BOX = 16      # the build's default (LSN_RV_SMALL_BOX of livescan3d_amd/csrc/render.hip): a larger box is drawn by a whole wave


def _rot(ax_deg, ay_deg):
    ax, ay = np.deg2rad(ax_deg), np.deg2rad(ay_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return ry @ rx


POSE_A = render_ref.pose_at(_rot(11.0, -23.0), [0.31, -0.17, 0.45])
VIEWS = (np.stack([INTR, INTR]), np.stack([IDENTITY, POSE_A]))
VERTEX = [("R", "u1"), ("G", "u1"), ("B", "u1"), ("A", "u1"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")]


class Case:
    """ticks: [(vertices, triangles or None)]; intr (V, 7), wt (V, 12), w, h: the views; points: the mode; view: the view the witness
    reads; kills: the mutants of render_ref_py.RULES whose output differs; noop: the case draws nothing; witness(case, res): asserts that
    the case reaches what it is named for, res[k] = (depth, rgb, info, terms) of tick k in `view`; plan: the sensor size of the plan the
    GPU test uploads it to; fill: the byte behind every tick's vertices there."""

    def __init__(self, ticks, witness, kills=(), points=False, view=0, noop=False, views=VIEWS, size=(W, H), plan=(64, 48), fill=0):
        self.ticks, self.witness, self.kills, self.points, self.view, self.noop = ticks, witness, tuple(kills), points, view, noop
        self.intr, self.wt = (np.asarray(a, np.float32) for a in views)
        self.w, self.h = size
        self.plan, self.fill = plan, fill
        self.every_view = False      # True: the witness reads every view, res[k][q]


def _colors(seed, n):
    return np.random.default_rng(9000 + seed).integers(0, 256, (n, 3))


def at_uvz(uvz, colors=None, intr7=INTR):
    """Vertices at image positions (u, v) and depth Z (metres) of the identity camera: X = (u - cx) Z / fx, Y = (cy - v) Z / fy."""
    uvz = np.asarray(uvz, dtype=np.float64).reshape(-1, 3)
    cx, cy, fx, fy = (float(v) for v in intr7[:4])
    v = np.zeros(len(uvz), dtype=VERTEX)
    with np.errstate(all="ignore"):
        v["X"], v["Y"], v["Z"], v["A"] = (uvz[:, 0] - cx) * uvz[:, 2] / fx, (cy - uvz[:, 1]) * uvz[:, 2] / fy, uvz[:, 2], 255
    c = _colors(len(uvz), len(uvz)) if colors is None else np.asarray(colors).reshape(-1, 3)
    v["R"], v["G"], v["B"] = c[:, 0], c[:, 1], c[:, 2]
    return v


def posed(verts, wt=POSE_A, intr7=INTR, w=W, h=H):
    """The same camera-frame vertices seen from the camera of pose wt: p_world = R (p_cam + t).  Asserts that they project onto the
    integers they had under the identity."""
    wt64 = np.asarray(wt, np.float64)
    p = np.stack([verts["X"], verts["Y"], verts["Z"]], axis=1).astype(np.float64)
    q = (p + wt64[:3]) @ wt64[3:].reshape(3, 3).T
    out = verts.copy()
    out["X"], out["Y"], out["Z"] = q[:, 0], q[:, 1], q[:, 2]
    a, b = render_ref.project_view(verts, intr7, IDENTITY, w, h), render_ref.project_view(out, intr7, wt, w, h)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    return out


def oriented(p, q, r):
    """Three (x, y, d) corners in the winding the half-space test draws (den < 0), as one row of drawTriangle's nine numbers."""
    den = (q[1] - r[1]) * (p[0] - r[0]) + (r[0] - q[0]) * (p[1] - r[1])
    assert den != 0
    return [*p, *q, *r] if den < 0 else [*p, *r, *q]


def _soup(rows, colors=None):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 9)
    return render_ref.soup(rows, INTR, _colors(len(rows), 3 * len(rows)) if colors is None else colors)


def per_pixel(T, w=W, h=H, where=None):
    """Candidates per pixel of a terms record (where: a mask over the candidates)."""
    p = T["cy"] * w + T["cx"]
    return np.bincount(p if where is None else p[where], minlength=w * h).reshape(h, w)


# ---- projection edges -----------------------------------------------------------------------------------------------------------------

# (u, v, Z) -> the (x, y, d, drawable) DESIGN section 14 gives it
_NOT = (INT_MIN, INT_MIN, 0, False)
PROJ_POINTS = [
    ((-1.5, 2, 1.0), (-1, 2, 1000, False)), ((-1.4, 3, 1.0), (0, 3, 1000, True)), ((-0.6, 4, 1.0), (0, 4, 1000, True)),
    ((-0.5, 5, 1.0), (0, 5, 1000, True)), ((-0.4, 6, 1.0), (0, 6, 1000, True)),
    ((W - 1.6, 7, 1.0), (30, 7, 1000, True)), ((W - 1.5, 8, 1.0), (31, 8, 1000, True)), ((W - 0.6, 9, 1.0), (31, 9, 1000, True)),
    ((W - 0.5, 10, 1.0), (32, 10, 1000, False)), ((W - 0.4, 11, 1.0), (32, 11, 1000, False)),
    ((4.5, 13, 1.0), (5, 13, 1000, True)), ((5.5, 14, 1.0), (6, 14, 1000, True)),      # k + 0.5, k even and odd
    ((2, -1.5, 1.0), (2, -1, 1000, False)), ((3, -1.4, 1.0), (3, 0, 1000, True)), ((4, -0.6, 1.0), (4, 0, 1000, True)),
    ((5, -0.5, 1.0), (5, 0, 1000, True)), ((6, -0.4, 1.0), (6, 0, 1000, True)),
    ((7, H - 1.6, 1.0), (7, 22, 1000, True)), ((8, H - 1.5, 1.0), (8, 23, 1000, True)), ((9, H - 0.6, 1.0), (9, 23, 1000, True)),
    ((10, H - 0.5, 1.0), (10, 24, 1000, False)), ((11, H - 0.4, 1.0), (11, 24, 1000, False)),
    ((13, 4.5, 1.0), (13, 5, 1000, True)), ((14, 5.5, 1.0), (14, 6, 1000, True)),
    ((12, 16, -1.0), (12, 16, 0, False)), ((13, 16, -0.0), _NOT), ((14, 16, 0.0), _NOT), ((15, 16, 0.00099), (15, 16, 0, False)),
    ((16, 16, 0.001), (16, 16, 1, True)), ((17, 16, 0.0015), (17, 16, 1, True)), ((18, 16, 65.5349), (18, 16, 65534, True)),
    ((19, 16, 65.535), (19, 16, 65535, True)), ((20, 16, 70.0), (20, 16, 65535, True)),
]
# a NaN or an inf in one coordinate: the rotation carries it into the other two (0 * inf = NaN), nothing is left to draw
PROJ_NOT_FINITE = [(np.nan, 0.1, 1.0), (0.1, np.nan, 1.0), (0.1, 0.1, np.nan), (np.inf, 0.1, 1.0), (0.1, np.inf, 1.0), (0.1, 0.1, np.inf)]


def _w_expect(table, first=0):
    def w(c, res):
        T = res[0][3]
        for g, (_, (x, y, d, ok)) in enumerate(table, first):
            assert (int(T["x"][g]), int(T["y"][g]), int(T["d"][g]), bool(T["ok"][g])) == (x, y, d, ok), (g, table[g - first])
    return w


def proj_points():
    v = at_uvz([p for p, _ in PROJ_POINTS])
    bad = np.zeros(len(PROJ_NOT_FINITE), dtype=VERTEX)
    for g, (x, y, z) in enumerate(PROJ_NOT_FINITE):
        bad[g] = (7 * g + 1, 200, 100, 255, x, y, z)
    table = PROJ_POINTS + [(p, _NOT) for p in PROJ_NOT_FINITE]

    def w(c, res):
        _w_expect(table)(c, res)
        assert res[0][2]["drawn"] == sum(e[3] for _, e in table) == res[0][2]["pixels"]

    # (x_le_w and y_le_h are killed by `drawn` alone here: the vertex on x == w or y == h has no pixel to show in)
    return Case([(np.concatenate([v, bad]), None)], w, points=True,
                kills=("project_floor", "project_rint", "x_le_w", "y_le_h", "d0_drawable", "d_wraps", "d_abs", "points_clamped"))


# triangles of (u, v) corners at 1 m; `drawn`: the definition draws it
PROJ_CORNERS = [
    (((-1.4, 3), (-0.6, 9), (6, 3)), ((0, 3), (0, 9), (6, 3)), True), (((-1.5, 12), (0, 18), (6, 12)), ((-1, 12), (0, 18), (6, 12)), False),
    (((25, 3), (25, 9), (W - 0.6, 3)), ((25, 3), (25, 9), (31, 3)), True), (((25, 12), (25, 18), (W - 0.5, 12)), ((25, 12), (25, 18), (32, 12)), False),
    (((10, -1.4), (10, 5), (16, -0.5)), ((10, 0), (10, 5), (16, 0)), True), (((10, 18), (10, H - 0.5), (16, 18)), ((10, 18), (10, 24), (16, 18)), False),
    (((18, 18), (18, H - 0.6), (23, 18)), ((18, 18), (18, 23), (23, 18)), True), (((18, 8), (18.5, 14), (23.5, 8)), ((18, 8), (19, 14), (24, 8)), True),
]


def proj_corners():
    v = at_uvz([(u, w_, 1.0) for uv, _, _ in PROJ_CORNERS for u, w_ in uv])
    table = [((u, w_, 1.0), (x, y, 1000, 0 <= x < W and 0 <= y < H)) for uv, xy, _ in PROJ_CORNERS for (u, w_), (x, y) in zip(uv, xy)]

    def w(c, res):
        _w_expect(table)(c, res)
        assert res[0][3]["keep"].tolist() == [d for _, _, d in PROJ_CORNERS] and res[0][2]["pixels"] > 40

    return Case([(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3))], w, kills=("project_floor", "project_rint", "x_le_w", "y_le_h"))


# triangles of (u, v, Z) corners -> the (x, y, d, drawable) of each; the rest of the listed edge values, the Z edges and what is not finite
_B = 1.0      # a plain corner: 1 m
PROJ_CORNERS_Z = [
    (((-0.4, 2, _B), (1, 8, _B), (7, 2, _B)), ((0, 2, 1000, True), (1, 8, 1000, True), (7, 2, 1000, True))),
    (((W - 8, 2, _B), (W - 8, 8, _B), (W - 1.6, 2, _B)), ((24, 2, 1000, True), (24, 8, 1000, True), (30, 2, 1000, True))),
    (((W - 8, 10, _B), (W - 8, 16, _B), (W - 1.5, 10, _B)), ((24, 10, 1000, True), (24, 16, 1000, True), (31, 10, 1000, True))),
    (((W - 8, 17, _B), (W - 8, 22, _B), (W - 0.4, 17, _B)), ((24, 17, 1000, True), (24, 22, 1000, True), (32, 17, 1000, False))),
    (((9, -0.4, _B), (9, 6, _B), (14, -1.4, _B)), ((9, 0, 1000, True), (9, 6, 1000, True), (14, 0, 1000, True))),
    (((9, 14, _B), (9, H - 1.6, _B), (14, 14, _B)), ((9, 14, 1000, True), (9, 22, 1000, True), (14, 14, 1000, True))),
    (((16, 14, _B), (16, H - 1.5, _B), (21, 14, _B)), ((16, 14, 1000, True), (16, 23, 1000, True), (21, 14, 1000, True))),
    (((1, 14, _B), (1, H - 0.4, _B), (6, 14, _B)), ((1, 14, 1000, True), (1, 24, 1000, False), (6, 14, 1000, True))),
    (((16, 2, 0.001), (16, 8, 0.001), (22, 2, 0.0015)), ((16, 2, 1, True), (16, 8, 1, True), (22, 2, 1, True))),
    (((1, 9, 65.535), (1, 13, 65.5349), (7, 9, 70.0)), ((1, 9, 65535, True), (1, 13, 65534, True), (7, 9, 65535, True))),
    (((9, 8, _B), (9, 12, _B), (14, 8, 0.00099)), ((9, 8, 1000, True), (9, 12, 1000, True), (14, 8, 0, False))),
    (((16, 9, _B), (16, 13, _B), (22, 9, -1.0)), ((16, 9, 1000, True), (16, 13, 1000, True), (22, 9, 0, False))),
    (((16, 9, _B), (16, 13, _B), (22, 9, 0.0)), ((16, 9, 1000, True), (16, 13, 1000, True), _NOT)),
    (((16, 9, _B), (16, 13, _B), (22, 9, -0.0)), ((16, 9, 1000, True), (16, 13, 1000, True), _NOT)),
]


def proj_corners_z():
    """The remaining edge values of u and v, the Z edges and NaN / inf in each coordinate, as corners of triangles: the triangle is drawn
    iff the three are drawable."""
    uvz = [c for corners, _ in PROJ_CORNERS_Z for c in corners]
    expect = [e for _, es in PROJ_CORNERS_Z for e in es]
    v = at_uvz(uvz)
    for x, y, z in PROJ_NOT_FINITE:      # a whole triangle (16, 9), (16, 13) and the corner that is not finite
        bad = at_uvz([(16, 9, _B), (16, 13, _B), (22, 9, _B)])
        bad["X"][2], bad["Y"][2], bad["Z"][2] = x, y, z
        v = np.concatenate([v, bad])
        expect += [(16, 9, 1000, True), (16, 13, 1000, True), _NOT]
    table = list(zip([None] * len(expect), expect))
    drawn = [all(e[3] for e in expect[k:k + 3]) for k in range(0, len(expect), 3)]

    def w(c, res):
        _w_expect(table)(c, res)
        assert res[0][3]["keep"].tolist() == drawn and sum(drawn) == 8 and res[0][2]["drawn"] == 8 and res[0][2]["pixels"] > 60
        assert {1, 65534, 65535} <= set(res[0][0].ravel().tolist())      # the triangle at 1 mm and the one at and beyond 65.535 m show

    return Case([(v, np.arange(len(v), dtype=np.int32).reshape(-1, 3))], w,
                kills=("project_floor", "project_rint", "x_le_w", "y_le_h", "d0_drawable", "d_abs", "d_wraps", "any_vertex"))


def proj_posed():
    """What of proj_points survives a rotation (no position exactly on a half), seen from POSE_A."""
    table = [(p, e) for p, e in PROJ_POINTS if all(abs(2 * c - round(2 * c)) > 0.1 or c == round(c) for c in p[:2]) and p[2] in (1.0, 0.0015, -1.0, 70.0)]
    assert len(table) == 15
    mid = lambda z: 1.0005 if z == 1.0 else z      # the middle of the millimetre: 1000 on the dot does not survive a rotation
    return Case([(posed(at_uvz([(u, v, mid(z)) for (u, v, z), _ in table])), None)], _w_expect(table), points=True, view=1,
                kills=("project_floor", "project_rint", "points_clamped", "d_abs", "d_wraps"))


# ---- one vertex out ---------------------------------------------------------------------------------------------------------------------

def _vertex_out(with_good):
    """Triangles of 5 x 5 px at 1000.5 mm on a grid of places; in the bad ones the named corners are off the image (u = -3), behind the camera
    (Z = -1 at the same pixel) or closer than 1 mm (Z = 0.5 mm)."""
    OFF, BEHIND, ZERO = "off", "behind", "zero"
    plan = [((2, 2), ()), ((10, 2), ((0, OFF),)), ((18, 2), ((1, BEHIND),)), ((25, 2), ((2, ZERO),)), ((2, 10), ((0, ZERO), (1, OFF))),
            ((10, 10), ((1, ZERO), (2, BEHIND))), ((18, 10), ((0, BEHIND), (1, OFF), (2, ZERO))), ((25, 10), ()), ((10, 17), ((2, BEHIND),))]
    uvz, good, bad_vertices = [], [], []
    for (x0, y0), bad in plan:
        if not bad and not with_good:
            continue
        corners = [[x0, y0, 1.0005], [x0, y0 + 5, 1.0005], [x0 + 5, y0, 1.0005]]
        for k, kind in bad:
            bad_vertices.append(len(uvz) + k)
            if kind == OFF:
                corners[k][0] = -3.0
            else:
                corners[k][2] = -1.0 if kind == BEHIND else 0.0005
        uvz += corners
        good.append(not bad)
    return at_uvz(uvz), np.arange(len(uvz), dtype=np.int32).reshape(-1, 3), good, bad_vertices


def _w_vertex_out(good, bad_vertices):
    def w(c, res):
        T, info = res[0][3], res[0][2]
        assert T["keep"].tolist() == good and info["drawn"] == sum(good)
        assert not T["ok"][bad_vertices].any() and int((~T["ok"]).sum()) == len(bad_vertices)
        assert {int(T["d"][g]) for g in bad_vertices} == {0, 1000}      # d = 0 behind and at the camera, 1000 off the image
        assert ((T["x"][bad_vertices] >= 0) & (T["d"][bad_vertices] == 0)).any()      # only d == 0 keeps it out
    return w


def vertex_out():
    v, t, good, bad = _vertex_out(True)
    return Case([(v, t)], _w_vertex_out(good, bad), kills=("any_vertex", "d0_drawable"))


def vertex_out_only():
    v, t, good, bad = _vertex_out(False)
    return Case([(v, t)], _w_vertex_out(good, bad), kills=("any_vertex", "d0_drawable"), noop=True)


def vertex_out_posed():
    v, t, good, bad = _vertex_out(True)
    return Case([(posed(v), t)], _w_vertex_out(good, bad), view=1, kills=("any_vertex", "d0_drawable"))


def index_out():
    rows = [[2, 2, 900, 2, 9, 900, 9, 2, 900], [12, 2, 800, 12, 9, 800, 19, 2, 800], [22, 2, 700, 22, 9, 700, 29, 2, 700], [2, 12, 600, 2, 19, 600, 9, 12, 600]]
    v, t = _soup(rows)
    nv = len(v)
    tris = np.array([t[0], [0, 1, nv], t[1], [-1, 4, 5], [6, 2 ** 30, 8], t[2], [nv, nv + 1, nv + 2], [3, 10, -2 ** 31], t[3]], dtype=np.int32)

    def w(c, res):
        assert res[0][3]["keep"].tolist() == [True, False, True, False, False, True, False, False, True] and res[0][2]["drawn"] == 4

    return Case([(v, tris)], w, kills=("index_clamped",))


# ---- winding and degenerate -----------------------------------------------------------------------------------------------------------

def _w_winding(n_front):
    def w(c, res):
        T, info = res[0][3], res[0][2]
        assert (T["den"] < 0).sum() == n_front and (T["den"] > 0).sum() == 2 and info["drawn"] == n_front + 2      # drawable, but nothing of them shows
        assert set(T["ck"].tolist()) == set(range(n_front))
    return w


MIRRORS = [[14, 2, 800, 22, 2, 800, 14, 10, 800], [16, 14, 300, 28, 20, 900, 20, 21, 500]]


def winding():
    return Case([_soup([[2, 2, 800, 2, 10, 800, 10, 2, 800], [2, 13, 300, 6, 20, 500, 14, 19, 900]] + MIRRORS)], _w_winding(2), kills=("both_windings",))


def _posed_twin(c):
    """The same case seen through POSE_A: its witness reads view 1."""
    return Case([(posed(v), t) for v, t in c.ticks], c.witness, kills=c.kills, points=c.points, view=1, noop=c.noop)


def winding_posed():
    return _posed_twin(winding())


def mirror_only():
    return Case([_soup(MIRRORS)], _w_winding(0), kills=("both_windings",), noop=True)


def degenerate():
    rows = [[2, 2, 500, 6, 6, 600, 10, 10, 700], [12, 2, 500, 12, 2, 500, 20, 8, 700], [5, 15, 500, 5, 15, 500, 5, 15, 500], [2, 20, 400, 10, 20, 500, 20, 20, 600],
            [25, 2, 400, 25, 9, 500, 25, 20, 600]]

    def w(c, res):
        T, info = res[0][3], res[0][2]
        assert not T["den"].any() and not info["boxes"].any() and info["drawn"] == 5 and len(T["ck"]) == 0

    # (den0_drawn is killed by `boxes` alone: every val of such a triangle is 0, no image can show it; on the GPU it is `large`, 4 here)
    return Case([_soup(rows)], w, kills=("den0_drawn",), noop=True)


def one_pixel():
    rows = [[5, 5, 700, 5, 6, 700, 6, 5, 700], [9, 9, 650, 10, 10, 650, 10, 9, 650], [20, 5, 600, 20, 6, 640, 21, 6, 660]]

    def w(c, res):
        T, info = res[0][3], res[0][2]
        assert info["boxes"].tolist() == [1, 1, 1] and T["ck"].tolist() == [0, 1, 2] and info["pixels"] == 3
        assert list(zip(T["cx"].tolist(), T["cy"].tolist())) == [(5, 5), (9, 9), (20, 5)]

    return Case([_soup(rows)], w, kills=("box_closed",))


def thin():
    rows = [[3, 3, 700, 3, 12, 900, 4, 3, 800], [8, 3, 650, 8, 4, 700, 20, 3, 900], [8, 8, 300, 20, 9, 400, 20, 8, 500], [25, 4, 300, 25, 20, 400, 26, 4, 350]]

    def w(c, res):
        T, info = res[0][3], res[0][2]
        assert info["boxes"].tolist() == [9, 12, 12, 16] and np.bincount(T["ck"]).tolist() == [9, 12, 12, 16]

    return Case([_soup(rows)], w, kills=("box_closed",))


# ---- fill rule -------------------------------------------------------------------------------------------------------------------------

# A shared edge P-Q with an apex either side: horizontal, vertical, both diagonals, slope 1/3; and how many of the two triangles have a
# pixel of the edge as a candidate.  drawTriangle's convention is not the watertight top-left rule: every edge value is a multiple of 256
# (integer corners in 28.4), so the C++ never changes a ">= 0", and a pixel on an edge belongs to both sides.  What keeps a horizontal or
# vertical shared edge single is the half-open box; on any other shared edge both triangles are candidates and the z-buffer decides.
SHARED = [((2, 5), (9, 5), (5, 2), (5, 9), 1), ((14, 2), (14, 9), (11, 5), (18, 5), 1), ((21, 2), (28, 9), (28, 2), (21, 9), 2),
          ((2, 19), (9, 12), (2, 12), (9, 19), 2), ((12, 14), (21, 17), (18, 11), (15, 21), 2)]


def _on_segment(p, q):
    """The integer points strictly between p and q."""
    n = int(np.gcd(q[0] - p[0], q[1] - p[1]))
    return [(p[0] + (q[0] - p[0]) * k // n, p[1] + (q[1] - p[1]) * k // n) for k in range(1, n)]


def shared_edges():
    rows = []
    for k, (p, q, s, t, _) in enumerate(SHARED):
        rows += [oriented((*p, 400 + 20 * k), (*q, 410 + 20 * k), (*s, 405 + 20 * k)), oriented((*q, 700 + 20 * k), (*p, 710 + 20 * k), (*t, 705 + 20 * k))]

    def w(c, res):
        depth, _, _, T = res[0]
        n = per_pixel(T)
        on_an_edge = set()
        for k, (p, q, _, _, sides) in enumerate(SHARED):
            between = _on_segment(p, q)
            on_an_edge |= set(between) | {p, q}
            assert len(between) >= 2 and all(n[y, x] == sides for x, y in between), (p, q)
            assert sides == 1 or all(399 + 20 * k <= depth[y, x] <= 410 + 20 * k for x, y in between)      # the nearer of the two
        assert {(int(x), int(y)) for y, x in zip(*np.nonzero(n > 1))} <= on_an_edge      # no other pixel has two candidates

    return Case([_soup(rows)], w, kills=("edge_gt",))


def shared_edges_posed():
    return _posed_twin(shared_edges())


def fan8():
    cx, cy = 16, 12
    ring = [(4, 0), (4, 4), (0, 4), (-4, 4), (-4, 0), (-4, -4), (0, -4), (4, -4)]
    rows = [oriented((cx, cy, 900), (cx + ring[k][0], cy + ring[k][1], 900), (cx + ring[(k + 1) % 8][0], cy + ring[(k + 1) % 8][1], 900)) for k in range(8)]

    def w(c, res):
        T = res[0][3]
        n = per_pixel(T)
        inner = n[cy - 4:cy + 4, cx - 4:cx + 4]      # the half-open square the eight cover
        assert (inner >= 1).all() and n.sum() == inner.sum()
        ys, xs = np.nonzero(n == 2)      # two candidates: on a diagonal spoke alone (the spokes along x and y are single: half-open boxes)
        assert n.max() == 2 and n[cy, cx] == 2 and len(ys) >= 8 and (np.abs(xs - cx) == np.abs(ys - cy)).all()
        # where two of them meet the vals are equal (flat d) and the lower index shows
        for q in np.flatnonzero(n.ravel() == 2):
            at = np.flatnonzero(T["cy"] * W + T["cx"] == q)
            if len(set(T["cval"][at].tolist())) == 1:
                assert T["wk"][T["wp"] == q][0] == T["ck"][at].min()

    return Case([_soup(rows)], w, kills=("edge_gt", "tie_higher"))


# ---- val at its edges ------------------------------------------------------------------------------------------------------------------

def _spread(seed, n, d, x1=30, y1=22):
    """n triangles of the drawn winding with corners inside 2 .. x1 - 1 by 2 .. y1 - 1; d(rng) -> the three corner depths."""
    rng = np.random.default_rng(seed)
    rows = []
    while len(rows) < n:
        p = np.stack([rng.integers(2, x1, 3), rng.integers(2, y1, 3)], axis=1)
        if (p[1, 1] - p[2, 1]) * (p[0, 0] - p[2, 0]) + (p[2, 0] - p[1, 0]) * (p[0, 1] - p[2, 1]) != 0:
            dd = d(rng)
            rows.append(oriented((*p[0], dd[0]), (*p[1], dd[1]), (*p[2], dd[2])))
    return rows


def _w_val_zero(values, least):
    def w(c, res):
        depth, _, info, T = res[0]
        assert set(T["cval"].tolist()) == set(values)
        zero_only = (per_pixel(T) > 0) & (per_pixel(T, where=T["cval"] != 0) == 0)
        assert zero_only.sum() >= least and not depth[zero_only].any()      # covered, and empty
        assert info["pixels"] == int((per_pixel(T, where=T["cval"] != 0) > 0).sum()) > 10
    return w


def val_d1():
    return Case([_soup(_spread(31, 6, lambda rng: (1, 1, 1)))], _w_val_zero((0, 1), 10), kills=("val0_drawn", "val_round"))


def val_d12():
    return Case([_soup(_spread(51, 6, lambda rng: np.roll([1, 1, 2], rng.integers(0, 3))))], _w_val_zero((0, 1, 2), 1), kills=("val0_drawn", "val_round"))


FAR = [[0, 0, 500, 0, 23, 500, 31, 0, 500], [31, 23, 500, 31, 0, 500, 0, 23, 500]]      # the whole view, two triangles


def val_near_far():
    """d = 1 triangles stored ahead of and behind a far surface (d = 500) that covers the view."""
    near = _spread(77, 6, lambda rng: (1, 1, 1))

    def w(c, res):
        depth, _, _, T = res[0]
        is_near = (T["ck"] != 3) & (T["ck"] != 4)
        zero = (per_pixel(T, where=is_near & (T["cval"] == 0)) > 0) & (per_pixel(T, where=is_near & (T["cval"] != 0)) == 0)
        one = per_pixel(T, where=is_near & (T["cval"] == 1)) > 0
        far = per_pixel(T, where=~is_near) > 0
        assert (zero & far).sum() >= 8 and (one & far).sum() > 10
        assert (depth[zero & far] >= 499).all() and (depth[one] == 1).all()      # the far one shows through; the near one wins

    return Case([_soup(near[:3] + FAR + near[3:])], w, kills=("val0_drawn", "val_round"))


def val_near_far_posed():
    return _posed_twin(val_near_far())


def val_max():
    def w(c, res):
        assert set(res[0][3]["cval"].tolist()) == {65534, 65535} and (res[0][3]["d"] == 65535).all()

    return Case([_soup(_spread(34, 5, lambda rng: (65535, 65535, 65535)))], w, kills=("val_round",))


def _found(row, colors, rule):
    """One triangle, found by a search over random small triangles, on which `rule` changes a byte."""
    def w(c, res):
        T = res[0][3]
        assert len(T["wp"]) >= 3 and res[0][2]["pixels"] == len(T["wp"])

    return Case([_soup([row], colors)], w, kills=(rule,))


val_round = functools.partial(_found, [8, 7, 160, 6, 4, 113, 4, 2, 240], [[208, 166, 233], [128, 155, 248], [186, 161, 139]], "val_round")
val_fused = functools.partial(_found, [8, 6, 24477, 5, 2, 43034, 3, 7, 57667], [[165, 189, 156], [76, 18, 156], [63, 30, 147]], "val_fma")
w3_order = functools.partial(_found, [8, 6, 2246, 4, 2, 34327, 6, 9, 26882], [[1, 139, 197], [189, 250, 135], [151, 247, 81]], "w3_grouped")
den_recip = functools.partial(_found, [8, 6, 2246, 4, 2, 34327, 6, 9, 26882], [[1, 139, 197], [189, 250, 135], [151, 247, 81]], "recip_den")
color_order = functools.partial(_found, [6, 6, 500, 9, 3, 500, 5, 3, 500], [[215, 141, 20], [47, 224, 113], [241, 23, 67]], "color_sum_order")
color_fused = functools.partial(_found, [5, 2, 500, 8, 7, 500, 9, 2, 500], [[243, 37, 109], [112, 235, 20], [100, 12, 92]], "color_fma")


# ---- ties -----------------------------------------------------------------------------------------------------------------------------

TIE_A, TIE_B = [3, 8, 700, 9, 5, 700, 2, 5, 700], [9, 7, 700, 8, 5, 700, 2, 6, 700]      # found by search: three common pixels of one val
TIE_C = [2, 9, 700, 10, 6, 700, 4, 3, 700]
TIE_COLORS = {"A": [[250, 10, 10]] * 3, "B": [[10, 10, 250]] * 3, "C": [[10, 250, 10]] * 3}
TIE_ROWS = {"A": TIE_A, "B": TIE_B, "C": TIE_C}


def _w_tie(orders):
    def w(c, res):
        for k, order in enumerate(orders):
            depth, rgb, _, T = res[k]
            p = T["cy"] * W + T["cx"]
            tied = 0
            for q in np.unique(p):
                at = np.flatnonzero(p == q)
                if len(at) == len(order) and len(set(T["cval"][at].tolist())) == 1 and T["cval"][at[0]] != 0:
                    assert tuple(rgb[q // W, q % W]) == tuple(TIE_COLORS[order[0]][0]), (order, q)      # flat colours: the lower index's
                    tied += len(set(zip(T["cw1"][at].tolist(), T["cw2"][at].tolist()))) == len(order)      # different triangles: their weights differ here
            assert tied >= 1, order
            assert len({tuple(px) for px in rgb[depth != 0]}) == len(order)      # each of them shows somewhere
    return w


def _tie(orders):
    return [_soup([TIE_ROWS[n] for n in order], [c for n in order for c in TIE_COLORS[n]]) for order in orders]


def tie2_ab():
    return Case(_tie(["AB"]), _w_tie(["AB"]), kills=("tie_higher", "last_wins"))


def tie2_ba():
    return Case(_tie(["BA"]), _w_tie(["BA"]), kills=("tie_higher", "last_wins"))


TIE3_ORDERS = ["ABC", "BCA", "CAB", "CBA"]


def tie3():
    return Case(_tie(TIE3_ORDERS), _w_tie(TIE3_ORDERS), kills=("tie_higher", "last_wins"))


def zbuffer():
    """Triangle 1 has the nearest corner (d = 100) and is stored last, but over most of triangle 0 (flat, d = 500) it is the farther."""
    rows = [[2, 2, 500, 2, 14, 500, 14, 2, 500], [2, 2, 100, 2, 14, 900, 14, 2, 900]]

    def w(c, res):
        depth, _, _, T = res[0]
        assert (T["wk"] == 0).sum() > 20 and (T["wk"] == 1).sum() > 5 and depth[2, 2] == 100 and depth[8, 6] in (499, 500)

    return Case([_soup(rows, [[250, 10, 10]] * 3 + [[10, 10, 250]] * 3)], w, kills=("min_vertex_d", "last_wins"))


POINTS_TIE = sorted(set(itertools.permutations((7, 5, 5))))      # (5, 5, 7), (5, 7, 5), (7, 5, 5)


def _points_tie():
    """Three vertices on one pixel with d = 7, 5, 5 in every order (and two more pixels with the orders reversed in storage)."""
    xyd, want = [], []
    for j, ds in enumerate(POINTS_TIE + [p[::-1] for p in POINTS_TIE]):
        for d in ds:
            xyd.append((3 + 4 * j, 5 + 2 * j, d))
        want.append((3 + 4 * j, 5 + 2 * j, 3 * j + ds.index(5)))
    return render_ref.vertices_at(xyd, INTR, _colors(77, len(xyd))), want


def _w_points_tie(want):
    def w(c, res):
        depth, rgb, info, T = res[0]
        v = c.ticks[0][0]
        assert info["drawn"] == len(v) and info["pixels"] == len(want)
        for x, y, g in want:
            assert depth[y, x] == 5 and tuple(rgb[y, x]) == (v["R"][g], v["G"][g], v["B"][g])
            others = [k for k in range(len(v)) if (T["x"][k], T["y"][k]) == (x, y) and k != g]
            assert len(others) == 2 and all(tuple(rgb[y, x]) != (v["R"][k], v["G"][k], v["B"][k]) for k in others)
    return w


def points_tie():
    v, want = _points_tie()
    return Case([(v, None)], _w_points_tie(want), points=True, kills=("points_tie_higher", "points_last_wins"))


def points_posed():
    v, want = _points_tie()
    return Case([(posed(v), None)], _w_points_tie(want), points=True, view=1, kills=("points_tie_higher", "points_last_wins"))


# ---- colour ---------------------------------------------------------------------------------------------------------------------------

# found by search: a colour sum exactly on k + 0.5 with k even; one a rounding below a half; one a rounding above
HALF_ROWS = [[6, 4, 500, 8, 2, 500, 3, 4, 500], [12, 8, 500, 15, 8, 500, 13, 4, 500], [22, 17, 500, 26, 15, 500, 22, 12, 500]]
HALF_COLORS = [[146, 104, 33], [11, 0, 12], [38, 255, 48], [225, 47, 16], [95, 173, 31], [222, 87, 58], [50, 219, 97], [244, 132, 193], [157, 184, 101]]


def color_half():
    def w(c, res):
        v = res[0][3]["v"].astype(np.float64)
        frac = v - np.floor(v) - 0.5
        assert ((frac == 0) & (np.floor(v) % 2 == 0)).any()      # + 0.5 and truncation: k + 1; rint: k
        assert ((frac < 0) & (frac > -2e-5)).any() and ((frac > 0) & (frac < 2e-5)).any()

    return Case([_soup(HALF_ROWS, HALF_COLORS)], w, kills=("color_rint",))


def color_half_posed():
    return _posed_twin(color_half())


def color_channels():
    cols = [[10, 100, 200], [50, 150, 250], [90, 30, 170]]

    def w(c, res):
        rgb = res[0][1][res[0][0] != 0]
        assert len(rgb) > 20 and (rgb[:, 0] != rgb[:, 2]).all() and len({tuple(p) for p in rgb}) > 10

    return Case([_soup([[3, 3, 900, 5, 20, 600, 28, 8, 300]], cols)], w, kills=("color_bgr", "color_flat"))


EXTREME_ROWS = [[2, 2, 500, 2, 11, 500, 13, 4, 500], [16, 2, 500, 16, 11, 500, 29, 4, 500], [2, 13, 500, 2, 22, 500, 13, 15, 500], [16, 13, 500, 16, 22, 500, 29, 15, 500]]
EXTREME_COLORS = [[255] * 3] * 3 + [[0] * 3] * 3 + [[255] * 3, [255] * 3, [0, 255, 0]] + [[0] * 3, [0] * 3, [255, 0, 255]]


def color_extremes():
    """0 and 255 at all three corners and at two of them; the third corner's weight is negative on some pixels of the edge opposite it
    (a rounding below zero).  Nothing leaves [0, 255]: the clamp has no witness (see render_ref_py.RULES)."""
    def w(c, res):
        depth, rgb, _, T = res[0]
        assert (_winner_w3(T) < 0).sum() >= 1
        by = {k: rgb.reshape(-1, 3)[T["wp"][T["wk"] == k]] for k in range(4)}
        assert (by[0] == 255).all() and (by[1] == 0).all() and len(by[0]) > 10 and len(by[1]) > 10
        assert (T["v"] > -0.5).all() and (T["v"] < 255.5).all() and (T["v"] > 255).any() and (T["v"] < 0).any()

    return Case([_soup(EXTREME_ROWS, EXTREME_COLORS)], w)


def _winner_w3(T):
    """w3 of every winning pixel (the candidates of a soup without overlap are the winners, val 0 aside)."""
    key = {(int(k), int(y) * W + int(x)): float(w3) for k, x, y, w3 in zip(T["ck"], T["cx"], T["cy"], T["cw3"])}
    return np.array([key[(int(k), int(p))] for k, p in zip(T["wk"], T["wp"])])


# ---- small or large box -----------------------------------------------------------------------------------------------------------------

BOX_SHAPES = [((1, 15), (1, 1)), ((1, 16), (3, 1)), ((1, 17), (5, 1)), ((15, 1), (8, 1)), ((16, 1), (8, 3)), ((17, 1), (8, 5)), ((3, 5), (8, 8)), ((4, 4), (13, 8)), ((2, 8), (19, 8))]


def _box_row(k):
    (bw, bh), (x0, y0) = BOX_SHAPES[k]
    return [x0, y0, 400 + 30 * k, x0, y0 + bh, 420 + 30 * k, x0 + bw, y0, 440 + 30 * k]


def _w_boxes(c, res):
    boxes = np.concatenate([r[2]["boxes"] for r in res])
    assert boxes.tolist() == [bw * bh for (bw, bh), _ in BOX_SHAPES] and sorted(set(boxes.tolist())) == [15, 16, 17]
    assert int((boxes > SMALL_BOX).sum()) == 2 and all(r[2]["pixels"] > 0 for r in res)


def boxes_together():
    return Case([_soup([_box_row(k) for k in range(len(BOX_SHAPES))])], _w_boxes)


def boxes_posed():
    return _posed_twin(boxes_together())


def boxes_apart():
    return Case([_soup([_box_row(k)]) for k in range(len(BOX_SHAPES))], _w_boxes)


# ---- more listed triangles than waves --------------------------------------------------------------------------------------------------

INTR_64 = render_ref.intrinsics(64, 48)
VIEWS_64 = (np.stack([INTR_64, INTR_64]), np.stack([IDENTITY, POSE_A]))
WAVES_LAUNCHED = 96      # the 64 x 48 plan: 6144 triangle slots, 24 workgroups of four waves


def waves():
    rng = np.random.default_rng(41)
    rows = []
    while len(rows) < 240:
        p = np.stack([rng.integers(0, 64, 3), rng.integers(0, 48, 3)], axis=1)
        if np.ptp(p[:, 0]) * np.ptp(p[:, 1]) > SMALL_BOX and (p[1, 1] - p[2, 1]) * (p[0, 0] - p[2, 0]) + (p[2, 0] - p[1, 0]) * (p[0, 1] - p[2, 1]) != 0:
            d = rng.integers(300, 4000, 3)
            rows.append(oriented((*p[0], d[0]), (*p[1], d[1]), (*p[2], d[2])))
    cloud = render_ref.soup(rows, INTR_64, _colors(41, 720))

    def w(c, res):
        info, T = res[0][2], res[0][3]
        assert int((info["boxes"] > SMALL_BOX).sum()) == 240 > 2 * WAVES_LAUNCHED and per_pixel(T, 64, 48).max() > 20
        assert len(set(T["wk"].tolist())) > 60      # many of them show

    return Case([cloud], w, views=VIEWS_64, size=(64, 48), kills=("last_wins", "tie_higher", "min_vertex_d"))


# ---- scratch across views and ticks ----------------------------------------------------------------------------------------------------

def _tiles(n, seed, d0):
    """n x n squares of 3 x 3 px (two triangles each) in the middle of the 64 x 48 view: boxes of 9 px there, of 36 px at twice the focal length."""
    rng = np.random.default_rng(seed)
    rows = []
    for j in range(n):
        for i in range(n):
            x0, y0, d = 20 + 3 * i, 14 + 3 * j, d0 + int(rng.integers(0, 400))
            rows += [[x0, y0, d, x0, y0 + 3, d + 3, x0 + 3, y0, d + 5], [x0 + 3, y0, d + 5, x0, y0 + 3, d + 3, x0 + 3, y0 + 3, d + 8]]
    return render_ref.soup(rows, INTR_64, _colors(seed, 3 * len(rows)))


AWAY = render_ref.pose_at(np.diag([-1.0, 1.0, -1.0]), [0.0, 0.0, 0.0])      # turned about y by pi
ZOOM_64 = np.array([32, 24, 128, 128, 0, 0, 0], dtype=np.float32)
SCRATCH_VIEWS = (np.stack([ZOOM_64, INTR_64, INTR_64]), np.stack([IDENTITY, AWAY, IDENTITY]))


def _w_scratch(order):
    zoom, away, plain = order

    def w(c, res_all):
        """(this witness reads every view: res_all[k][q])"""
        for k in (0, 2):
            i = [res_all[k][q][2] for q in range(3)]
            assert i[zoom]["drawn"] == i[plain]["drawn"] > 30 and (i[zoom]["boxes"] > SMALL_BOX).all() and not (i[plain]["boxes"] > SMALL_BOX).any()
            assert i[away]["drawn"] == 0 and i[away]["pixels"] == 0 and i[zoom]["pixels"] > 3 * i[plain]["pixels"] > 0
        assert all(res_all[1][q][2]["drawn"] == 0 and res_all[1][q][2]["pixels"] == 0 for q in range(3))
        assert len(c.ticks[2][0]) < len(c.ticks[0][0])
    return w


def _scratch(order):
    ticks = [_tiles(7, 51, 900), (np.zeros(0, dtype=VERTEX), np.zeros((0, 3), np.int32)), _tiles(4, 52, 1500)]
    views = tuple(np.stack([a[q] for q in np.argsort(order)]) for a in SCRATCH_VIEWS)
    c = Case(ticks, _w_scratch(order), views=views, size=(64, 48), fill=0x5B)
    c.every_view = True
    return c


def scratch():
    return _scratch((0, 1, 2))


def scratch_reverse():
    """The view that lists nothing first, then the one that lists everything."""
    return _scratch((1, 0, 2))


SCRATCH_SMALL = (np.array([16, 12, 32, 32, 0, 0, 0], dtype=np.float32), IDENTITY, 32, 24)      # the same plan afterwards, mesh mode at a smaller view


def views16():
    """16 views of 8 x 6 px, every one another pose, on two ticks."""
    intr = render_ref.intrinsics(8, 6)
    rows0 = [[1, 1, 900, 1, 5, 950, 6, 1, 990], [6, 1, 700, 2, 5, 720, 7, 5, 740], [0, 0, 1200, 0, 5, 1200, 7, 0, 1200]]
    rows1 = [[2, 0, 500, 0, 4, 600, 6, 5, 700], [3, 2, 400, 3, 3, 400, 4, 2, 400]]
    ticks = [render_ref.soup(r, intr, _colors(60 + k, 3 * len(r))) for k, r in enumerate((rows0, rows1))]
    wts = [IDENTITY] + [render_ref.pose_at(_rot(0.8 * q - 6.0, 5.0 - 0.7 * q), [0.02 * q - 0.15, 0.1 - 0.015 * q, 0.02 * q - 0.1]) for q in range(1, 16)]
    assert len({w.tobytes() for w in wts}) == 16

    def w(c, res_all):
        shown = [res_all[k][q][2]["pixels"] for k in range(2) for q in range(16)]
        assert sum(p > 0 for p in shown) >= 16 and len(set(shown)) >= 6 and res_all[0][0][2]["drawn"] == 3

    c = Case(ticks, w, views=(np.tile(intr, (16, 1)), np.stack(wts)), size=(8, 6))
    c.every_view = True
    return c


# ---- more triangles than one pass of the raster grid -------------------------------------------------------------------------------------

RASTER_PLAN = (512, 257)                      # capacity 131584 vertices, 263168 triangles: 1028 tiles of 256 against 1024 workgroups
RASTER_ONE_PASS = 1024 * 256                  # what one pass of rv_raster_kernel's grid takes
RASTER_SLOTS = 2 * 512 * 257
RASTER_COUNTS = (RASTER_SLOTS - 37, RASTER_SLOTS)      # the last wave partly filled; the tick ends on a wave boundary
INTR_256 = render_ref.intrinsics(256, 256)


@functools.lru_cache(maxsize=None)
def raster_two_pass():
    """One vertex per pixel of a 256 x 256 view (depths 600 .. 3000) and 1002 more at d = 1, shared by both ticks.  Every triangle slot is
    filled with triangles of one to three pixels; among the last 1100 entries lie triangles of 10 x 10 px (listed), triangles of the
    d = 1 vertices and indices out of range."""
    rng = np.random.default_rng(71)
    ys, xs = np.mgrid[0:256, 0:256]
    grid = np.stack([xs.ravel(), ys.ravel(), 600 + (xs.ravel() * 7 + ys.ravel() * 13) % 2400], axis=1)
    base = np.stack([rng.integers(0, 250, 334), rng.integers(0, 250, 334), np.ones(334, np.int64)], axis=1)
    near = np.concatenate([base, base + [[0, 3, 0]], base + [[3, 0, 0]]])      # corner j, 334 + j, 668 + j: a triangle of 3 px legs at d = 1
    verts = render_ref.vertices_at(np.concatenate([grid, near]), INTR_256, rng.integers(0, 256, (256 * 256 + 1002, 3)))
    nv = len(verts)
    vid = lambda x, y: y * 256 + x
    ticks = []
    for k, nt in enumerate(RASTER_COUNTS):
        x, y, s = rng.integers(0, 253, nt), rng.integers(0, 253, nt), rng.integers(1, 3, nt)      # legs of 1 or 2 px: 1 or 3 pixels
        tris = np.stack([vid(x, y), vid(x, y + s), vid(x + s, y)], axis=1)
        tail = np.arange(nt - 1100, nt)[::-1]      # from the last entry down
        big = tail[::7]
        bx, by = rng.integers(0, 245, len(big)), rng.integers(0, 245, len(big))
        tris[big] = np.stack([vid(bx, by), vid(bx, by + 10), vid(bx + 10, by)], axis=1)
        one = tail[1::7][:120]
        j = rng.integers(0, 334, len(one))
        tris[one] = np.stack([256 * 256 + j, 256 * 256 + 334 + j, 256 * 256 + 668 + j], axis=1)
        bad = tail[2::7][:40]
        tris[bad, k % 3] = np.where(np.arange(len(bad)) % 2 == 0, nv + np.arange(len(bad)), -1 - np.arange(len(bad)))
        ticks.append((verts, tris.astype(np.int32)))

    def w(c, res):
        for k, nt in enumerate(RASTER_COUNTS):
            info, T = res[k][2], res[k][3]
            second = np.flatnonzero(T["keep"]) >= RASTER_ONE_PASS      # kept triangles that the grid's second pass draws
            assert nt > RASTER_ONE_PASS and second.sum() > 900 and (info["boxes"][second] > SMALL_BOX).sum() > 100
            assert (~T["keep"][RASTER_ONE_PASS:]).sum() == 40 and len(set(T["wk"][T["wk"] >= RASTER_ONE_PASS].tolist())) > 150
        assert RASTER_COUNTS[0] % 64 not in (0, 63) and RASTER_COUNTS[1] % 64 == 0 and RASTER_COUNTS[1] == RASTER_SLOTS
        assert len(c.ticks[0][0]) <= 512 * 257

    return Case(ticks, w, views=(INTR_256[None], IDENTITY[None]), size=(256, 256), plan=RASTER_PLAN)


# ---- the int32 budget ------------------------------------------------------------------------------------------------------------------

INTR_1024 = render_ref.intrinsics(1024, 1024)


@functools.lru_cache(maxsize=None)
def budget_1024():
    """Tick 0: (0,0)-(0,1023)-(1023,0) and its complement, in the drawn winding; tick 1: a sliver from (0,0) to (1023,1023) in front of
    them.  render_ref.walk asserts that no 28.4 product leaves int32."""
    a = [0, 0, 1000, 0, 1023, 3000, 1023, 0, 2000]
    b = [1023, 1023, 4000, 1023, 0, 2000, 0, 1023, 3000]
    sliver = [0, 0, 500, 1022, 1023, 700, 1023, 1023, 900]
    ticks = [render_ref.soup(r, INTR_1024, _colors(81 + k, 3 * len(r))) for k, r in enumerate(([a, b], [a, sliver, b]))]

    def w(c, res):
        (d0, _, i0, T0), (d1, _, i1, T1) = res[0], res[1]
        assert i0["boxes"].tolist() == [1023 * 1023] * 2 and i0["pixels"] == 1023 * 1023 and not d0[1023].any() and not d0[:, 1023].any()
        ys, xs = np.nonzero(per_pixel(T0, 1024, 1024) > 1)      # the shared diagonal belongs to both (see SHARED)
        assert len(ys) > 1000 and (xs + ys == 1023).all() and (T0["den"] == -1023 * 1023).all()
        assert (T1["wk"] == 1).sum() >= 400 and i1["boxes"][1] == 1023 * 1023 and T1["den"][1] == -1023

    return Case(ticks, w, views=(INTR_1024[None], IDENTITY[None]), size=(1024, 1024))


BUILDERS = {
    "proj_points": proj_points, "proj_corners": proj_corners, "proj_corners_z": proj_corners_z, "proj_posed": proj_posed,
    "vertex_out": vertex_out, "vertex_out_only": vertex_out_only, "vertex_out_posed": vertex_out_posed, "index_out": index_out,
    "winding": winding, "winding_posed": winding_posed, "mirror_only": mirror_only, "degenerate": degenerate, "one_pixel": one_pixel, "thin": thin,
    "shared_edges": shared_edges, "shared_edges_posed": shared_edges_posed, "fan8": fan8,
    "val_d1": val_d1, "val_d12": val_d12, "val_near_far": val_near_far, "val_near_far_posed": val_near_far_posed, "val_max": val_max, "val_round": val_round, "val_fused": val_fused,
    "w3_order": w3_order, "den_recip": den_recip,
    "tie2_ab": tie2_ab, "tie2_ba": tie2_ba, "tie3": tie3, "zbuffer": zbuffer, "points_tie": points_tie, "points_posed": points_posed,
    "color_half": color_half, "color_half_posed": color_half_posed, "color_channels": color_channels, "color_extremes": color_extremes,
    "color_order": color_order, "color_fused": color_fused,
    "boxes_together": boxes_together, "boxes_posed": boxes_posed, "boxes_apart": boxes_apart, "waves": waves,
    "scratch": scratch, "scratch_reverse": scratch_reverse, "views16": views16,
    "raster_two_pass": raster_two_pass, "budget_1024": budget_1024,
}
NAMES = tuple(BUILDERS)
# No plain-loop twin for these two: a Python loop over 2^20 pixels (budget_1024) or 263168 triangles twice (raster_two_pass) is minutes.
NUMPY_ONLY = ("raster_two_pass", "budget_1024")
# What the GPU test draws as the ticks of one plan (same views, same size); the others have a test of their own.
GROUPED = tuple(n for n in NAMES if n not in NUMPY_ONLY + ("scratch", "scratch_reverse", "views16"))


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()
