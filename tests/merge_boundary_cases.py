"""Rigs that drive the overlay merge to its decision boundaries (test infrastructure): tests/test_merge_boundary_ref.py holds every rig
to what it claims on the CPU (a census through merge_ref's trace, and the mutants of merge_ref.RULES each rig kills),
tests/golden/merge_boundary_ref.npz holds the reference's own output on them, tests/test_merge_boundary_gpu.py runs them on the GPU.

Every rig is a synth.Rig of 2 or 3 equal-sized sensors, 64 x 48 unless its name says otherwise, with R = I poses (so that a sensor's
pixel grid maps onto another's by its intrinsics alone) and integer principal points (so that a projected position k + 0.5 is never at a
rounding boundary unless the rig wants it there):

  zero_*        magnified same-pose pairs (sensor 1's focal length 3 and 2.5 times sensor 0's) at depths 1, 1..2 and 1..3 mm: base 1
                sees sensor 0's pixel triangles magnified, with interior pixels whose interpolated depth truncates to 0 (zero writers),
                and the inclusive edge test (CX >= 0 on both sides of a shared edge) puts two writers on every shared edge pixel and up
                to six on a shared vertex.  Half of base 1 lies at 20 mm: there |base - mapped| < 20 holds for val 1..3 and fails for
                val 0, so the winner of a pixel decides its mask.  Base 0 sees sensor 1 minified: several vertices per pixel, thousands
                of den == 0 triangles (`degenerate`), zero-area boxes.  zero_roll_d3: the same with sensor 1 rolled by 180 degrees and
                a little beside sensor 0 (see zero_roll).
  discard_*     sensor 1 magnifies by 4, is rolled by 180 degrees and lies (-0.1, -0.04, -0.2) mm from sensor 0, whose depths are 1..6 mm: the
                2 mm vertices come back as d = 1 (flat patches of them give zero writers) while deeper layers fold over them, so that
                some pixels have a writer with a small non-zero val BEFORE the last zero writer and a larger val behind it
                (merge_ref.SMALLER_DISCARDED: the t > zmax filter must throw the earlier one away).  Base 1 lies at 15 mm, where every
                val 0..6 passes the depth test, except at those pixels (DISCARD_PIXELS, found by search and held by the census): there
                it is the discarded val + 20 or 21, which the true winner passes and the discarded writer would fail -- the mask, and with it
                the merged map, depends on the filter.
  den0          same intrinsics, sensor 1 (depths 1..3 mm) 0.06 / 0.03 mm beside sensor 0 (a plateau at 21 mm): the parallax shears sensor
                1's pixel triangles, many collapse onto diagonals whose box holds pixels, and base 0 at 21 passes val 2..3 and fails the
                val 0 that a drawn den == 0 triangle would leave (`degenerate`: the skip decides outputs).
  thresholds    same pose, same intrinsics: sensor 1 a plateau, sensor 0 the plateau with isolated probes at +-18, +-19, +-20, +-21,
                at least 6 pixels apart and 3 from the border (`depth_threshold`): a probe's verdict decides its own 5 x 5 block after
                the two erosions.  The mask is false on the whole border (see below) and the erosions carry that two pixels inwards.
  far           the same at 65510 / 65535: the probes and the plateau reach the u16 ceiling.
  confidence    two plateaus, single zero pixels in the overlay's raw map: the confidence ramp around them puts tags 4, 5, 6, 7 on
                plateau pixels whose depth test passes (`conf_threshold`).
  shared_*      magnifications 3 and 2 at 1500 mm +- 3 with a few holes (tags vary from triangle to triangle) and, in the base, 4 % of
                the pixels 17, 20 or 23 mm off: shared edges and vertices pass exactly through pixel centres, for the four edge classes
                of the fill convention, and sensor 1's principal point puts magnified vertices into its last column and row.
  shift         sensor 1's principal point 3 pixels right and 4 down of sensor 0's (the triangulation leaves a margin of up to 3 pixels
                without triangles): sensor 0's vertices land in base 1 at x = w - 1, w and y = h - 1, h, sensor 1's in base 0 at
                x = 0, 1 and y = 0, 1, each with triangles that lose exactly one vertex (`project_drop`).
  near_zero     sensor 1 0.6 mm in front of sensor 0 at depths 1..2 mm: sensor 0's 1 mm vertices project into base 1 with d == 0
                (dropped), its 2 mm vertices with d == 1 (`project_drop`, d == 0).
  wobble        one sensor translated by (300 m, 0, 0.3 m) at depths 1..3 mm: float32 rounding of X + 300 is wider than a pixel there, so
                its OWN reprojection puts several vertices on one pixel, moves others out of the frame, and turns 1 mm into d == 0
                (`reproject_collide`); a second sensor with the same pose makes it a merge.
  feedback      three sensors, same pose and intrinsics: sensor 1 agrees with sensor 0 on the left two thirds, sensor 2 on the right two
                thirds.  What base 0 assigns is missing from sensor 0 as an overlay of bases 1 and 2, and the overlap of the two masks
                is eroded differently when the overlays are visited in the other order (`assigned_feedback`).
  tiny_WxH      three equal plateaus on 2 x 8, 8 x 2, 8 x 4, 4 x 8, 6 x 7 and 8 x 9 frames.  Below 3 columns or 5 rows the triangulation
                makes no triangle, so nothing is mapped and the mask is empty (2 x 8, 8 x 2, 8 x 4); 4 x 8 has a raw mask that the first
                erosion removes, 6 x 7 one that the second removes, 8 x 9 is the smallest frame that assigns a vertex.

What this entry point cannot reach, and why:
  * cvt_u16_x64's wrap of values outside 0..65535: the projected depths are clamped to 0..65535 and the weights of a covered pixel
    are convex up to rounding, so val stays within [0, 65535.x]; tests/test_merge_ref.py drives the conversion itself.
  * the fill convention's increment (:644-646): every projected position is an integer, so every edge function is a multiple of 256
    and C + 1 >= 0 exactly when C >= 0.  The increment can change no pixel here (no mutant for it: it could be killed by no rig);
    render.hip's copy is driven with fractional positions by its own tests.
  * a mask that is true on the frame's border (`erode_border`): mapDepthMap drops vertices with x < 1 or y < 1, so nothing covers row 0
    or column 0; it keeps x = w - 1 and y = h - 1, but drawTriangle's box is half-open (maxx = ceil of the largest x, exclusive), so
    nothing is drawn into the last column or row either (shared_* put vertices there and the census finds them uncovered).  An uncovered
    pixel has tag 0 and fails the mask.  "morphologyErode leaves the border as it is" therefore always keeps a false border, and the
    mutant that clears it (merge_ref.UNDECIDED_RULES "border_cleared") changes nothing.  tests/test_merge_ref.py holds erode to the
    reference's own morphologyErode on masks with a true border.
  * point_assigned in mapDepthMap (:860): a vertex is assigned exactly when the pixel that owns it is zeroed, and a zeroed pixel makes
    no triangle, so an assigned vertex is never in a triangle of the overlay's CURRENT maps.  Ignoring point_assigned ("assigned_ignored")
    changes nothing; what feeds back from base to base is the zeroed depth, and `feedback` holds that.
  * SMALLER_DISCARDED with sensors at one pose: on one surface every writer of a pixel interpolates the same depth, so the zero_* rigs
    have none (the census says so); the discard_* rigs reach it with folded layers.
  * more than 32 sensors: refused (tests/test_merge_boundary_gpu.py::test_more_than_32_sensors_are_refused).
  * sensors of different sizes: refused (tests/test_overlay_merge_gpu.py::test_mixed_sizes_rejected)."""
import functools

import numpy as np

from livescan3d_amd import synth

W, H = 64, 48
HUGE_BOUNDS = np.array([-1e6, -1e6, -1e6, 1e6, 1e6, 1e6], dtype=np.float32)
IDENTITY = (np.eye(3), np.zeros(3))
PROBE_OFFSETS = (18, 19, 20, 21, -18, -19, -20, -21)
PROBE_XY = [(10, 14), (22, 14), (34, 14), (46, 14), (10, 30), (22, 30), (34, 30), (46, 30)]


def _intr(f, cx, cy):
    return np.float32([cx, cy, f, f, 0, 0, 0])


def _rig(depths, focals, seed, poses=None, centres=None):
    rng = np.random.default_rng(1000 + seed)
    h, w = depths[0].shape
    centres = centres or [(w // 2, h // 2)] * len(depths)
    poses = poses or [IDENTITY] * len(depths)
    return synth.Rig([np.asarray(d, dtype=np.uint16) for d in depths], [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in depths],
                     np.concatenate([_intr(f, *c) for f, c in zip(focals, centres)]), np.concatenate([synth.pack_pose(*p) for p in poses]),
                     HUGE_BOUNDS)


def comes_back(d):
    """What depth d comes back as from createVertices + pointProjection under an identity pose: (int)(float(d) / 1000.0f * 1000.0f)."""
    return int(np.float32(np.float32(d) / np.float32(1000.0)) * np.float32(1000.0))


def roundtrips(d):
    return comes_back(d) == d


def plateau_level(lo):
    """The first level >= lo that comes back exactly together with every probe around it."""
    p = lo
    while not all(roundtrips(p + k) for k in (0,) + PROBE_OFFSETS):
        p += 1
    return p


def zero_val(mag, top, seed):
    rng = np.random.default_rng(seed)
    d0 = rng.integers(1, top + 1, (H, W))
    d1 = rng.integers(1, top + 1, (H, W))
    d1[:, :W // 2] = 20
    return _rig([d0, d1], [50.0, 50.0 * mag], seed)


def zero_roll(mag, top, seed):
    """Sensor 1 rolled by 180 degrees about the optical axis (R = diag(-1, -1, 1), exact) and 40 / 20 micrometres beside sensor 0: the
    magnified triangles arrive in the opposite raster order, so the zero writer of a shared edge is often the LAST one, and parallax
    folds 2 x 2 blocks of depths 1..top over one another."""
    rng = np.random.default_rng(seed)
    d0 = np.kron(rng.integers(1, top + 1, (H // 2, W // 2)), np.ones((2, 2), dtype=np.int64))
    d1 = rng.integers(1, 4, (H, W))
    d1[:, :W // 2] = 20
    return _rig([d0, d1], [50.0, 50.0 * mag], seed, poses=[IDENTITY, (np.diag([-1.0, -1.0, 1.0]), np.array([4e-5, 2e-5, 0.0]))])


DISCARD_POSE = (np.diag([-1.0, -1.0, 1.0]), np.array([-1e-4, -4e-5, -2e-4]))
# seed: [(x, y in base 1, the discarded val, the winner's val)]
DISCARD_PIXELS = {215: [(15, 6, 2, 3), (17, 6, 2, 4)], 24: [(11, 36, 1, 3)]}


def discard(seed):
    rng = np.random.default_rng(seed)
    d0 = rng.integers(1, 7, (H, W))
    d1 = np.full((H, W), 15)
    for x, y, a, win in DISCARD_PIXELS[seed]:
        d1[y, x] = a + (21 if win - a > 1 else 20)      # within [a + 20, win + 19] as it comes back (the census holds it)
    return _rig([d0, d1], [50.0, 200.0], seed, poses=[IDENTITY, DISCARD_POSE])


def den0():
    rng = np.random.default_rng(41)
    return _rig([np.full((H, W), 21), rng.integers(1, 4, (H, W))], [50.0, 50.0], 41,
                poses=[IDENTITY, (np.eye(3), np.array([6e-5, -3e-5, 0.0]))])


def thresholds(w=W, h=H, level=1500, probes=True, seed=7):
    p = plateau_level(level)
    d0 = np.full((h, w), p)
    if probes:
        for (x, y), k in zip(PROBE_XY, PROBE_OFFSETS):
            d0[y, x] = p + k
    return _rig([d0, np.full((h, w), p)], [50.0, 50.0], seed)


FAR_LEVELS = (65510, 65535)
FAR_PROBES = [((8, 12), 18), ((20, 12), 19), ((8, 30), 20), ((20, 30), 21), ((46, 12), -18), ((56, 12), -19), ((46, 30), -20), ((56, 30), -21)]


def far():
    """Overlay: 65510 on the left, 65535 on the right; base: the same with probes 18 .. 21 above on the left and below on the right.
    (Float32 has 256 steps per metre there, so only some millimetres come back as themselves: 65516 + 18 does not, 65510 + 18 .. 21 and
    65535 - 18 .. 21 do; `roundtrips` is asserted for every level used.)"""
    d1 = np.full((H, W), FAR_LEVELS[0])
    d1[:, W // 2:] = FAR_LEVELS[1]
    d0 = d1.copy()
    for (x, y), k in FAR_PROBES:
        d0[y, x] += k
    assert all(roundtrips(int(d)) for d in np.unique(d0))
    return _rig([d0, d1], [50.0, 50.0], 8)


def confidence():
    p = plateau_level(1500)
    d0, d1 = np.full((H, W), p), np.full((H, W), p)
    for x, y in [(16, 16), (44, 14), (30, 34), (52, 36)]:
        d1[y, x] = 0
    return _rig([d0, d1], [50.0, 50.0], 9)


def shared_edges(mag, centre, seed):
    """centre: sensor 1's principal point, chosen so that magnified vertices land in its last column and row."""
    rng = np.random.default_rng(seed)
    d0 = 1500 + rng.integers(-3, 4, (H, W))
    for x, y in [(30, 22), (35, 26), (28, 27)]:
        d0[y, x] = 0
    d1 = 1500 + rng.integers(-3, 4, (H, W))
    far_off = rng.random((H, W)) < 0.04
    d1[far_off] += rng.choice([-23, -20, -17, 17, 20, 23], int(far_off.sum()))
    return _rig([d0, d1], [50.0, 50.0 * mag], seed, centres=[(W // 2, H // 2), centre])


def shift():
    p = plateau_level(1500)
    return _rig([np.full((H, W), p), np.full((H, W), p)], [50.0, 50.0], 10, centres=[(W // 2, H // 2), (W // 2 + 3, H // 2 + 4)])


def near_zero():
    rng = np.random.default_rng(11)
    d0 = rng.integers(1, 3, (H, W))
    d1 = rng.integers(1, 3, (H, W))
    return _rig([d0, d1], [50.0, 50.0], 11, poses=[IDENTITY, (np.eye(3), np.array([0.0, 0.0, 0.0006]))])


def wobble():
    rng = np.random.default_rng(12)
    pose = (np.eye(3), np.array([300.0, 0.0, 0.3]))
    return _rig([rng.integers(1, 4, (H, W)), rng.integers(1, 4, (H, W))], [50.0, 50.0], 12, poses=[pose, pose], centres=[(30, H // 2)] * 2)


def feedback():
    p = plateau_level(1500)
    d0 = np.full((H, W), p)
    d1, d2 = d0.copy(), d0.copy()
    d1[:, 40:] = p + 40
    d2[:, :24] = p + 40
    return _rig([d0, d1, d2], [50.0] * 3, 13)


def tiny(w, h):
    p = plateau_level(1500)
    return _rig([np.full((h, w), p)] * 3, [50.0] * 3, 14 + w)


TINY_SIZES = ((2, 8), (8, 2), (8, 4), (4, 8), (6, 7), (8, 9))

BUILDERS = {
    "zero_m3_d1": lambda: zero_val(3.0, 1, 1), "zero_m3_d2": lambda: zero_val(3.0, 2, 2), "zero_m3_d3": lambda: zero_val(3.0, 3, 3),
    "zero_m2.5_d1": lambda: zero_val(2.5, 1, 4), "zero_m2.5_d2": lambda: zero_val(2.5, 2, 5), "zero_m2.5_d3": lambda: zero_val(2.5, 3, 6),
    "zero_roll_d3": lambda: zero_roll(3.0, 3, 3),
    "discard_215": lambda: discard(215), "discard_24": lambda: discard(24), "den0": den0,
    "thresholds": thresholds, "far": far, "confidence": confidence,
    "shared_m3": lambda: shared_edges(3.0, (33, 26), 21), "shared_m2": lambda: shared_edges(2.0, (33, 25), 22),
    "shift": shift, "near_zero": near_zero, "wobble": wobble, "feedback": feedback,
    **{f"tiny_{w}x{h}": functools.partial(tiny, w, h) for w, h in TINY_SIZES},
}
NAMES = tuple(BUILDERS)
DIGEST_ONLY = ("feedback", "shared_m3")      # the fixture keeps sha256 and count of these rigs' triangles, the arrays of the others


def equals_fixture(z, name, tris):
    """tris (m, 3) int32 are the reference's triangles of rig `name` in the loaded fixture z."""
    import hashlib
    tris = np.ascontiguousarray(tris, dtype="<i4")
    if name in DIGEST_ONLY:
        return len(tris) == int(z[name + "/n_triangles"]) and hashlib.sha256(tris.tobytes()).hexdigest() == str(z[name + "/triangles_sha256"])
    want = z[name + "/triangles"]
    return tris.shape == want.shape and np.array_equal(tris, want)

# The mutants of merge_ref.RULES that each rig is built to kill (tests/test_merge_boundary_ref.py holds every entry).
_ZERO = ("zero_writers_ignored", "k_ge_z")
_THRESHOLDS = ("depth_threshold_19", "depth_threshold_21")
_CONF = ("conf_threshold_4", "conf_threshold_6")
KILLS = {
    "zero_m3_d1": _ZERO + ("drop_gt_wh",), "zero_m3_d2": _ZERO, "zero_m3_d3": _ZERO, "zero_m2.5_d1": _ZERO, "zero_m2.5_d2": _ZERO,
    "zero_m2.5_d3": ("one_dropped_vertex_drawn",), "zero_roll_d3": _ZERO + ("one_dropped_vertex_drawn",),
    "discard_215": ("nonzero_minimum",), "discard_24": ("nonzero_minimum",), "den0": ("den0_drawn",),
    "thresholds": _THRESHOLDS + ("one_erosion",), "far": _THRESHOLDS, "confidence": _CONF,
    "shared_m3": _THRESHOLDS + _CONF, "shared_m2": _THRESHOLDS + _CONF,
    "shift": ("drop_lt_0", "drop_gt_wh"), "near_zero": ("drop_lt_0", "drop_gt_wh", "one_dropped_vertex_drawn"),
    "wobble": ("reproject_d0_test", "first_vertex_wins"), "feedback": ("overlays_decreasing", "one_erosion"),
    "tiny_2x8": (), "tiny_8x2": (), "tiny_8x4": (), "tiny_4x8": (), "tiny_6x7": ("one_erosion",), "tiny_8x9": ("one_erosion",),
}
ZERO_VAL = tuple(n for n in NAMES if n.startswith("zero_"))


@functools.lru_cache(maxsize=None)
def rig(name):
    return BUILDERS[name]()
