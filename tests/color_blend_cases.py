"""Hand-made rigs for the colour blend across views (csrc/color_blend.hip; the definition: tests/color_blend_ref.py).  Test infrastructure.
tests/test_color_blend_ref.py holds every case to its witness on the definition alone -- what the case is named for is reached -- and to
the mutants of color_blend_ref_py.RULES it is listed to kill; tests/test_color_blend_gpu.py runs the cases on the GPU.

As in tests/color_boundary_cases.py, unless a case says otherwise every sensor stands at the identity pose with the intrinsics
(cx, cy, f) = (w // 2, h // 2, 50) and a flat frame at 1500 mm: a pixel reprojects onto itself, a flat frame has no seed (confidence 20
everywhere) and a zero pixel in the interior makes the confidence ramp 1, 2, 3 .. around it.  No frame is larger than 65 x 65.

  one_sensor, no_overlap      no-ops: one sensor; two sensors 50 m apart.
  rounding                    8 x 6 twice, flat colours, a hole in sensor 1: with weights 20 and 1 .. 4 the channels put
                              sum + floor(W / 2) on a multiple of W, one below and one above.
  tol_edge                    depth_tol 10: sensor 1 lies 9 mm behind sensor 0 on its left half, 10 mm on its right.
  conf_edge                   min_confidence 5: the ramp around a hole in sensor 1 puts 4 and 5 under sensor 0's vertices; sensor 1's own
                              vertices beside the hole blend at confidence 1.
  crop_hole                   the crop box's z-min removes all but 7 of sensor 0's vertices: sensor 1 finds depth without a vertex.
  proj_shift                  sensor 1 stands 1.6 pixels right of and below sensor 0: projections onto -1, 0, w - 1, w (and h).
  behind, far, nan_pose       d1 == 0 behind the camera on a pixel that would match; d1 clamped at 65535; a NaN in sensor 1's pose.
  three                       three sensors see one patch: the three-term mean.
  jacobi                      two sensors, colour gradients, a hole: reading a colour already blended changes a byte.
  after_transfer              64 x 48 twice with a colour gain: the colour transfer runs first and the blend reads what it wrote.
  size_1x1 .. size_65x33, mixed   frame sizes around the confidence pass's 32-pixel tile; three sizes in one rig.
  count_255 .. count_257      that many vertices in the tick; sensor 0 has 100, so the sensor boundary lies inside a wave.
  two_ticks                   two ticks of one plan with different holes and colours.
  n32                         32 sensors of 4 x 4, R = 255 at weight 20 everywhere: the largest sum, 32 * 20 * 255.
  off_tol0, off_conf21        no-ops: the parameters that switch the stage off.  min_conf0: 0 is read as 1.
  alpha                       alpha bytes 0, 255 and a pattern.
33 sensors are refused (rig33)."""
import functools

import numpy as np

from livescan3d_amd import synth
from tests import color_cases
from tests.color_boundary_cases import L0, _flat, _intr, _pixels

WIDE = color_cases.WIDE_BOUNDS


def _rig(depths, colors, shifts=None, intrs=None, bounds=WIDE, wts=None):
    """colors: per sensor an (h, w, 3) array, one (r, g, b) for the whole frame, or an int: the seed of random colours."""
    depths = [np.asarray(d, dtype=np.uint16) for d in depths]
    rgbs = []
    for d, c in zip(depths, colors):
        if isinstance(c, (int, np.integer)):
            c = np.random.default_rng(7000 + int(c)).integers(0, 256, d.shape + (3,))
        rgbs.append(np.broadcast_to(np.asarray(c, dtype=np.uint8), d.shape + (3,)).copy())
    shifts = shifts or [np.zeros(3)] * len(depths)
    intrs = intrs or [_intr(d.shape[1], d.shape[0]) for d in depths]
    wts = wts or [synth.pack_pose(np.eye(3), t) for t in shifts]
    return synth.Rig(depths, rgbs, np.concatenate(intrs), np.concatenate(wts), bounds)


class Case:
    """ticks: the rigs of one plan; pre: what runs on the fused cloud in front of the blend (None, "transfer", "alpha"); noop: the case
    is named a no-op (nothing may change); kills: the mutants of color_blend_ref_py.RULES whose output differs."""

    def __init__(self, ticks, tol=15, minc=1, pre=None, noop=False, kills=()):
        self.ticks, self.tol, self.minc, self.pre, self.noop, self.kills = ticks, tol, minc, pre, noop, tuple(kills)


def _hole(d, x, y):
    d = d.copy()
    d[y, x] = 0
    return d


ROUND_COLORS = ((119, 5, 78), (92, 206, 4))      # R alone reaches all three; G lands on a multiple, B one below an odd W


def rounding():
    return Case([_rig([_flat(L0, 8, 6), _hole(_flat(L0, 8, 6), 3, 2)], ROUND_COLORS)], kills=("no_half", "half_ceil"))


def tol_edge():
    d1 = _flat(L0 + 9, 8, 6)
    d1[:, 4:] = L0 + 10
    return Case([_rig([_flat(L0, 8, 6), d1], (1, 2))], tol=10, kills=("tol_le", "no_abs"))


def conf_edge():
    return Case([_rig([_flat(L0, 16, 12), _hole(_flat(L0, 16, 12), 7, 5)], (3, 4))], minc=5, kills=("conf_gt", "conf_ge_m1", "own_gated"))


CROP_BOUNDS = np.array([-100, -100, 1.505, 100, 100, 100], dtype=np.float32)
CROP_KEPT = 7


def crop_hole():
    d0 = _flat(L0, 8, 6).ravel()
    d0[np.random.default_rng(11).permutation(48)[:CROP_KEPT]] = L0 + 20
    return Case([_rig([d0.reshape(6, 8), _flat(L0 + 10, 8, 6)], (5, 6), bounds=CROP_BOUNDS)], kills=("no_vertex_read",))


def proj_shift():
    t = np.array([_pixels(1.6), -_pixels(1.6), 0.0])
    return Case([_rig([_flat(L0, 16, 12), _flat(L0, 16, 12)], (7, 8), shifts=[np.zeros(3), t])], kills=("project_floor", "edge_inclusive"))


BW, BH = 64, 48
BEHIND_PATCH_X = 30                       # sensor 0: x < 30 lies at 10 mm
BEHIND_BLOCK = (22, 26, 44, 42)           # sensor 1: x0, y0, x1, y1 of a block that sees sensor 0's plateau


def behind():
    """Sensor 1 stands 0.9 m in front of sensor 0 and looks at a wall 0.5 m away -- behind sensor 0 (tz = -0.4: d1 = 0, the image
    mirrored) -- with a block at 3.9 m (tz = 3, sensor 0's plateau).  Sensor 0's left part lies at 10 mm: the wall's vertices land there
    with |0 - 10| < depth_tol, and d1 != 0 alone keeps them out."""
    d0 = _flat(3000, BW, BH)
    d0[:, :BEHIND_PATCH_X] = 10
    d1 = _flat(500, BW, BH)
    x0, y0, x1, y1 = BEHIND_BLOCK
    d1[y0:y1, x0:x1] = 3900
    return Case([_rig([d0, d1], (9, 10), shifts=[np.zeros(3), np.array([0.0, 0.0, -0.9])], intrs=[_intr(BW, BH), _intr(BW, BH, cx=20, cy=24)])],
                kills=("no_d1_test",))


def far():
    return Case([_rig([_flat(65530, BW, BH), _flat(65000, BW, BH)], (11, 12), shifts=[np.zeros(3), np.array([0.0, 0.0, 1.0])])], kills=("d_wraps",))


def nan_pose():
    wts = [synth.pack_pose(np.eye(3), np.zeros(3)) for _ in range(3)]
    wts[1][0] = np.nan      # t0 of sensor 1: its vertices' X is NaN, and every projection into it has a NaN x
    return Case([_rig([_flat(L0, 8, 6)] * 3, (13, 14, 15), wts=wts)], kills=("cvt_saturates",))


THREE_COLORS = ((10, 20, 30), (200, 100, 50), (77, 255, 0))


def three():
    return Case([_rig([_flat(L0, 8, 6)] * 3, THREE_COLORS)], kills=("lower_only",))


def _gradient(w, h, k):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 17 + k * 40) % 256, (y * 29 + k * 90) % 256, ((x + y) * 11 + k * 5) % 256], axis=-1)


def jacobi():
    return Case([_rig([_flat(L0, 12, 10), _hole(_flat(L0, 12, 10), 5, 4)], (_gradient(12, 10, 0), _gradient(12, 10, 3)))], kills=("gauss_seidel",))


def after_transfer():
    rng = np.random.default_rng(21)
    c0 = rng.integers(0, 256, (48, 64, 3))
    c1 = np.clip(c0 * 0.8 + 30 + rng.integers(-3, 4, c0.shape), 0, 255).astype(np.int64)
    return Case([_rig([_flat(L0), _flat(L0)], (c0, c1))], pre="transfer", kills=("raw_colors",))


SIZES = ((1, 1), (2, 2), (33, 33), (65, 33))


def size(w, h):
    d = _flat(L0, w, h)
    if w >= 33:
        d[h // 2, 31] = 0      # the ramp crosses the confidence tile's border at x = 32 (and y = 32 where the frame has it)
        d[h - 2, w - 2] = 0
    return Case([_rig([d, _flat(L0, w, h)], (30 + w, 31 + h))])


def mixed():
    return Case([_rig([_flat(L0, 33, 33), _hole(_flat(L0, 65, 33), 40, 20), _flat(L0, 2, 2)], (41, 42, 43))])


def count(total):
    d1 = _flat(L0, 16, 10)
    d1[0, 1:1 + 260 - total] = 0      # zeros on the first row: no vertex there
    return Case([_rig([_flat(L0, 10, 10), d1], (50 + total, 51 + total))])


def two_ticks():
    a = _rig([_hole(_flat(L0, 12, 10), 3, 3), _flat(L0, 12, 10)], (61, 62))
    b = _rig([_flat(L0, 12, 10), _hole(_hole(_flat(L0, 12, 10), 8, 6), 2, 7)], (63, 64))
    return Case([a, b], minc=3, kills=("tick0_index",))


def n32():
    cols = [(255, (s * 37) % 256, (s * 91 + 5) % 256) for s in range(32)]
    return Case([_rig([_flat(L0, 4, 4)] * 32, cols)], kills=("sum_16bit",))


def rig33():
    return _rig([_flat(L0, 4, 4)] * 33, list(range(33)))


def _two(seed):
    return _rig([_flat(L0, 8, 6), _hole(_flat(L0, 8, 6), 4, 3)], (seed, seed + 1))


BUILDERS = {
    "one_sensor": lambda: Case([_rig([_flat(L0, 8, 6)], (70,))], noop=True),
    "no_overlap": lambda: Case([_rig([_flat(L0, 8, 6)] * 2, (71, 72), shifts=[np.zeros(3), np.array([50.0, 0.0, 0.0])])], noop=True),
    "rounding": rounding, "tol_edge": tol_edge, "conf_edge": conf_edge, "crop_hole": crop_hole, "proj_shift": proj_shift,
    "behind": behind, "far": far, "nan_pose": nan_pose, "three": three, "jacobi": jacobi, "after_transfer": after_transfer,
    **{f"size_{w}x{h}": functools.partial(size, w, h) for w, h in SIZES}, "mixed": mixed,
    **{f"count_{t}": functools.partial(count, t) for t in (255, 256, 257)},
    "two_ticks": two_ticks, "n32": n32,
    "off_tol0": lambda: Case([_two(80)], tol=0, noop=True), "off_conf21": lambda: Case([_two(82)], minc=21, noop=True),
    "min_conf0": lambda: Case([_two(84)], minc=0, kills=("min0_off",)),
    "alpha": lambda: Case([_two(86)], pre="alpha", kills=("alpha_255",)),
}
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def alpha_pattern(n):
    """The alpha bytes the "alpha" case puts on the fused cloud: 0, 255, then a pattern."""
    a = (np.arange(n) * 7 % 256).astype(np.uint8)
    a[:1], a[1:2] = 0, 255
    return a


def start(c, k, orc):
    """The cloud tick k of case c hands to the blend: as fused, or as `pre` left it."""
    from tests import color_blend_ref, color_ref
    rig = c.ticks[k]
    if c.pre == "transfer":
        return color_ref.color_transfer(rig, orc)[0]
    v, _ = color_blend_ref.fused(color_blend_ref.sensors_of(rig, orc))
    if c.pre == "alpha":
        v["A"] = alpha_pattern(len(v))
    return v
