"""Rigs that drive the colour transfer (csrc/color.hip, csrc/cloud_index.hip) to its decision boundaries (test infrastructure):
tests/test_color_boundary_ref.py holds every rig to what it claims on the CPU (a census of what it reaches, and the mutants of
color_ref_py.RULES it kills), tests/golden/color_boundary_ref.npz holds the reference's own output on them,
tests/test_color_boundary_gpu.py runs them on the GPU.

Unless its name says otherwise a rig has 64 x 48 frames, every sensor at the identity pose with the intrinsics (cx, cy, f) =
(32, 24, 50), random colours and color_cases.WIDE_BOUNDS: a pixel reprojects onto itself, a flat frame has no seed (confidence 20
everywhere) and the coverage of two equal flat frames is the whole frame.  The level trick: depth levels exactly 20 mm apart make no seed
inside a frame (the seed test is > 20) and do not match across sensors (the match test is < 20), so the coverage of a pair is the number
of pixels at which both sensors hold the same level.

  cov_100 .. cov_108   sensor 1 agrees with sensor 0 on exactly that many pixels: 100 gives no pair, 101 the first pair; the sample
                       counts 101 .. 108 take every residue mod 8 (ct_fold_kernel's unrolled loop and its tail).  One calibration:
                       they are also the ticks of one plan (TICKS).
  ns_K                 K = 0, 1, 7, 8, 9, 15, 16, 17: sensor 0 flat at 1500 with K pixels at 1520, sensor 1 flat at 1510, the crop box's
                       z-min at 1.505 m: the coverage is the whole frame, the pair is chosen, and only K pixels of sensor 0 still have a
                       vertex -- exactly K samples (ns_0: means 0, scales 1, no byte changes).  DEFINED: the reference reads colors1[-3..-1].
  between              three sensors: 0 a plateau, 1 in bands 18, 19, 20, 21 above it, 2 in bands 18 .. 21 below: both depth tests across
                       sensors on both sides (and a tie between (0, 1) and (0, 2)).
  frame_steps          one frame twice: a hole (seeds beside it), 2 x 2 blocks 19 and 20 above and below the plateau within 3 pixels of the
                       seeds: the BFS enters the 19s and not the 20s.
  seed_steps           one frame twice: single pixels 20 and 21 above and below the plateau: 21 seeds, 20 does not.
  conf_i, conf_j       a zero pixel in sensor 0 alone / in sensor 1 alone: the confidence ramp 1, 2, .. around it puts 4 and 5 on the
                       projected pixel's side alone / on the vertex's own side alone.
  corridor             one frame twice: a one-pixel corridor at the plateau's level minus 20 (so that nothing beside it is within 20),
                       31 steps long, from a seed at (22, 24) across x = 32 and y = 32 to (31, 38): its pixels' levels are their distance
                       along it, 19 and the capped 20 among them, whatever tile they lie in.
  size_WxH             widths and heights 2, 3, 32, 33, 63, 64, 65: depth on the last row and column, holes beside the first and the last
                       ones: x == 0 and y == 0 keep 20, x == w - 1 and y == h - 1 are reached.
  proj_frac            sensor 1 0.7 pixel left of and above sensor 0: its first column and row project to (-1, 0) before the truncation,
                       which makes them 0, inside the frame.
  proj_over            sensor 1 0.6 pixel right of and below: its last column and row project to x == w and y == h, outside.
  proj_frame           sensor 1 63.2 pixels to the right: its first column alone lands in sensor 0 (coverage 48: no pair).
  far                  sensor 1 at 65 m, 1 m behind sensor 0, whose frame lies at 65530: d is clamped at 65535 and matches.
  d1zero               128 x 96.  Sensor 1 is 0.9 m in front of sensor 0 and looks at a wall 0.5 m away (behind sensor 0: tz = -0.4, the
                       image mirrored, d1 = 0) with a block at 3.9 m (tz = 3, matching sensor 0's plateau: the coverage).  Sensor 0's left
                       part lies at 10 mm: the wall's vertices project there with |d1 - d2| = 10 and are samples (:1454 has no d1 test)
                       while the coverage (:1409) rejects them.
  plane                the same with sensor 1 0.5 m in front: the wall lies in sensor 0's camera plane (tz == 0), x and y are +-inf or,
                       on the principal row and column, NaN: INT_MIN, outside.  (Where the conversion gave 0 for NaN the vertex of the
                       principal point would become a sample at pixel (0, 0).)
  tie_first            four sensors: 0 and 1 agree everywhere, 2 and 3 agree with them (and with each other) on 150 pixels: the first
                       branch chooses among four equal coverages, twice.
  tie_second           0 = 1 and 2 = 3 everywhere, 150 pixels in common across: the second branch chooses between two equal coverages.
  b1_gt_b2             (2, 3) first; the first branch then finds (2, 0), (2, 1) and (3, 1) equal at 500 and takes (2, 0): a pair with
                       b1 > b2, sensor 0 corrected from sensor 2.
  early_end            0 = 1; 2 and 3 share 2860 pixels and 50 with the first pair: the first branch's best is 50, not 0, so the second
                       branch is not run and (2, 3) is never chosen.
  n32                  32 sensors of 16 x 8 whose coverages are all between 106 and 128: 31 pairs, the bit 1u << 31, the full LDS table.

33 sensors are refused (tests/test_color_boundary_gpu.py); an alpha byte other than 255 cannot come out of the export (createVertices
writes 255) and is set on the device by the GPU test."""
import functools

import numpy as np

from livescan3d_amd import synth
from tests import color_cases
from tests.merge_boundary_cases import plateau_level

W, H, F = 64, 48, 50.0
WIDE = color_cases.WIDE_BOUNDS
L0 = 1500


def _intr(w=W, h=H, f=F, cx=None, cy=None):
    return np.float32([w // 2 if cx is None else cx, h // 2 if cy is None else cy, f, f, 0, 0, 0])


def _rig(depths, seed, shifts=None, intrs=None, bounds=WIDE):
    """shifts: per sensor the translation t of its pose (R = I): a vertex of sensor j lies at p + t_j - t_i in sensor i's frame."""
    rng = np.random.default_rng(2000 + seed)
    depths = [np.asarray(d, dtype=np.uint16) for d in depths]
    shifts = shifts or [np.zeros(3)] * len(depths)
    intrs = intrs or [_intr(d.shape[1], d.shape[0]) for d in depths]
    return synth.Rig(depths, [rng.integers(0, 256, d.shape + (3,)).astype(np.uint8) for d in depths], np.concatenate(intrs),
                     np.concatenate([synth.pack_pose(np.eye(3), t) for t in shifts]), bounds)


def _flat(level, w=W, h=H):
    return np.full((h, w), level, dtype=np.int64)


def _some(seed, k, w=W, h=H):
    """k pixels of a frame, as a mask."""
    m = np.zeros(w * h, dtype=bool)
    m[np.random.default_rng(3000 + seed).permutation(w * h)[:k]] = True
    return m.reshape(h, w)


def cov(k):
    d1 = _flat(L0 + 20)
    d1[_some(k, k)] = L0
    return _rig([_flat(L0), d1], k)


NS = (0, 1, 7, 8, 9, 15, 16, 17)
NS_BOUNDS = np.array([-100, -100, 1.505, 100, 100, 100], dtype=np.float32)


def ns(k):
    d0 = _flat(L0)
    d0[_some(500 + k, k)] = L0 + 20
    return _rig([d0, _flat(L0 + 10)], 500 + k, bounds=NS_BOUNDS)


BETWEEN_STEPS = (18, 19, 20, 21)


def between():
    p = plateau_level(L0)
    d1, d2 = _flat(p), _flat(p)
    for b, k in enumerate(BETWEEN_STEPS):
        d1[:, 16 * b:16 * b + 16] = p + k
        d2[:, 16 * b:16 * b + 16] = p - k
    return _rig([_flat(p), d1, d2], 601)


STEP_HOLE = (16, 16)
STEP_BLOCKS = {19: (19, 17), 20: (12, 14), -19: (19, 13), -20: (12, 18)}      # offset: the block's first (x, y)


def frame_steps():
    d = _flat(L0)
    d[STEP_HOLE[1], STEP_HOLE[0]] = 0
    for k, (x, y) in STEP_BLOCKS.items():
        d[y:y + 2, x:x + 2] = L0 + k
    return _rig([d, d], 602)


SEED_PROBES = {20: (16, 12), -20: (16, 36), 21: (48, 12), -21: (48, 36)}


def seed_steps():
    d = _flat(L0)
    for k, (x, y) in SEED_PROBES.items():
        d[y, x] = L0 + k
    return _rig([d, d], 603)


CONF_HOLE = (32, 24)


def conf_side(side):
    d = [_flat(L0), _flat(L0)]
    d[side][CONF_HOLE[1], CONF_HOLE[0]] = 0
    return _rig(d, 604 + side)


CORRIDOR_START = (22, 24)
CORRIDOR_MOVES = ((1, 0, 8), (0, 1, 5), (1, 0, 5), (0, 1, 6), (-1, 0, 4), (0, 1, 3))


def corridor_path():
    x, y = CORRIDOR_START
    path = [(x, y)]
    for dx, dy, k in CORRIDOR_MOVES:
        for _ in range(k):
            x, y = x + dx, y + dy
            path.append((x, y))
    return path


def corridor():
    d = _flat(L0 + 20)
    for x, y in corridor_path():
        d[y, x] = L0
    d[CORRIDOR_START[1] - 1, CORRIDOR_START[0] - 1] = 0     # the hole whose (1, 1) neighbour is the corridor's first pixel
    return _rig([d, d], 606)


SIZES = ((2, 65), (3, 64), (32, 33), (33, 32), (63, 3), (64, 2), (65, 63))


def size(w, h):
    d = _flat(L0, w, h)
    if w >= 5 and h >= 5:
        d[2, 2] = 0                  # seeds at (1, 1), beside the first row and column, and at (3, 3)
        d[h - 3, w - 3] = 0          # seeds at (w - 2, h - 2), beside the last row and column, and at (w - 4, h - 4)
    elif w >= 3 and h >= 3:
        d[0, 0] = 0                  # a zero on the border keeps 20 and seeds (1, 1)
        d[h - 1, w - 1] = 0          # ... and (w - 2, h - 2)
    return _rig([d, d], 610 + w)


def _pixels(px, z=L0 / 1000.0, f=F):
    """px pixels as metres at depth z."""
    return px * z / f


def proj(dx, dy, seed):
    """Sensor 1's pixels land dx to the right of and dy below their own position in sensor 0."""
    return _rig([_flat(L0), _flat(L0)], seed, shifts=[np.zeros(3), np.array([_pixels(dx), -_pixels(dy), 0.0])])


def far():
    return _rig([_flat(65530), _flat(65000)], 620, shifts=[np.zeros(3), np.array([0.0, 0.0, 1.0])])


BW, BH, BF = 128, 96, 100.0
BEHIND_PATCH_X = 60                       # sensor 0: x < 60 lies at 10 mm
BEHIND_BLOCK = (45, 52, 89, 85)           # sensor 1: x0, y0, x1, y1 of the block that carries the coverage
BEHIND_J = (40, 48)                       # sensor 1's principal point


def behind(dz, block_level, plateau, seed):
    d0 = _flat(plateau, BW, BH)
    d0[:, :BEHIND_PATCH_X] = 10
    d1 = _flat(500, BW, BH)
    x0, y0, x1, y1 = BEHIND_BLOCK
    d1[y0:y1, x0:x1] = block_level
    return _rig([d0, d1], seed, shifts=[np.zeros(3), np.array([0.0, 0.0, dz])],
                intrs=[_intr(BW, BH, BF), _intr(BW, BH, BF, *BEHIND_J)])


def _agree(level_else, mask):
    d = _flat(level_else)
    d[mask] = L0
    return d


def tie_first():
    s = _some(701, 150)
    return _rig([_flat(L0), _flat(L0), _agree(L0 + 20, s), _agree(L0 - 20, s)], 701)


def tie_second():
    s = _some(702, 150)
    return _rig([_flat(L0), _flat(L0), _agree(L0 + 20, s), _agree(L0 + 20, s)], 702)


def b1_gt_b2():
    s0, s1 = _some(703, 500), _some(704, 500)
    d3 = _flat(L0)
    d3[np.flatnonzero(s0 & ~s1)[:10] // W, np.flatnonzero(s0 & ~s1)[:10] % W] = L0 - 20     # sensor 3 differs from 2 where only 0 agrees
    return _rig([_agree(L0 + 20, s0), _agree(L0 + 20, s1), _flat(L0), d3], 703)


def early_end():
    d2 = _flat(L0 + 20)
    d2[:1, :50] = L0                  # 50 pixels in common with the first pair
    d3 = d2.copy()
    d3[40:44, :53] = L0 + 40          # 212 pixels apart from sensor 2, away from the L0 pixels
    return _rig([_flat(L0), _flat(L0), d2, d3], 705)


N32_W, N32_H = 16, 8


def n32():
    depths = []
    for s in range(32):
        d = _flat(L0, N32_W, N32_H).ravel()
        d[:(s * 7) % 23] = L0 + 20
        depths.append(d.reshape(N32_H, N32_W))
    return _rig(depths, 732)


BUILDERS = {
    **{f"cov_{k}": functools.partial(cov, k) for k in range(100, 109)},
    **{f"ns_{k}": functools.partial(ns, k) for k in NS},
    "between": between, "frame_steps": frame_steps, "seed_steps": seed_steps,
    "conf_i": functools.partial(conf_side, 0), "conf_j": functools.partial(conf_side, 1), "corridor": corridor,
    **{f"size_{w}x{h}": functools.partial(size, w, h) for w, h in SIZES},
    "proj_frac": lambda: proj(-0.7, -0.7, 615), "proj_over": lambda: proj(0.6, 0.6, 616), "proj_frame": lambda: proj(63.2, 0.0, 617),
    "far": far, "d1zero": lambda: behind(-0.9, 3900, 3000, 621), "plane": lambda: behind(-0.5, 3500, 3000, 622),
    "tie_first": tie_first, "tie_second": tie_second, "b1_gt_b2": b1_gt_b2, "early_end": early_end, "n32": n32,
}
NAMES = tuple(BUILDERS)
DEFINED = frozenset(f"ns_{k}" for k in NS)      # the reference reads out of bounds here: the restatements are the definition
FULL = ("cov_101", "size_2x65", "size_3x64", "size_63x3", "n32", "proj_frac")      # the fixture keeps these rigs' bytes, digests of the others


def equals_fixture(z, name, verts):
    """verts (VERTEX_DTYPE or bytes (n, 16)) are the reference's corrected vertices of rig `name` in the loaded fixture z."""
    import hashlib
    b = np.frombuffer(np.ascontiguousarray(verts).tobytes(), np.uint8).reshape(-1, 16)
    if len(b) != int(z[name + "/n_vertices"]) or hashlib.sha256(b.tobytes()).hexdigest() != str(z[name + "/vertices_sha256"]):
        return False
    return name not in FULL or np.array_equal(z[name + "/vertices"], b)


TAIL = tuple(f"cov_{k}" for k in range(101, 109))
# ticks of one plan (one size, one calibration): the tail rigs, cov_100 between them, and rigs whose confidence maps differ
TICKS = ("cov_101", "corridor", "cov_102", "cov_103", "cov_100", "conf_i", "cov_104", "cov_105", "frame_steps", "cov_106", "cov_107",
         "conf_j", "cov_108", "seed_steps")

# The mutants of color_ref_py.RULES that each rig is built to kill (tests/test_color_boundary_ref.py holds every entry).
KILLS = {
    **{f"cov_{k}": ("fold_tail_dropped",) if k % 8 else () for k in range(101, 109)},
    "cov_100": ("coverage_gt_99",), "cov_101": ("coverage_gt_101", "fold_tail_dropped"),
    **{f"ns_{k}": ("fold_tail_dropped",) if k % 8 else () for k in NS}, "ns_0": ("empty_scale_0",),
    "ns_1": (),      # (one sample is its own mean: the deviation is 0 with and without it)
    "between": ("cov_lt_19", "cov_lt_21", "smp_lt_19", "smp_lt_21", "second_branch_last_tie"),
    "frame_steps": ("bfs_lt_19", "bfs_lt_21"), "seed_steps": ("seed_gt_19", "seed_gt_21"),
    "conf_i": ("conf_i_ge_4", "conf_i_ge_6"), "conf_j": ("conf_j_ge_4", "conf_j_ge_6"),
    "corridor": ("bfs_one_sweep_less", "bfs_lt_21"),
    **{f"size_{w}x{h}": ("border_low_visited", "border_high_skipped") if min(w, h) >= 3 else () for w, h in SIZES},
    "proj_frac": ("project_floor",), "proj_over": ("edge_inclusive",), "proj_frame": ("edge_inclusive",), "far": ("d_wraps",),
    "d1zero": ("smp_d1_test", "cov_no_d1_test"), "plane": ("cvt_saturates",),
    "tie_first": ("first_branch_last_tie",), "tie_second": ("second_branch_last_tie",),
    "b1_gt_b2": ("pair_sorted", "first_branch_last_tie"), "early_end": ("first_branch_falls_through",), "n32": ("bit_31_lost",),
}


@functools.lru_cache(maxsize=None)
def rig(name):
    return BUILDERS[name]()


def frames(r):
    """[(h, w) u16] of a rig."""
    dm, out, po = r.depth_maps.view("<u2"), [], 0
    for w, h in zip(r.widths.tolist(), r.heights.tolist()):
        out.append(dm[po:po + w * h].reshape(h, w))
        po += w * h
    return out


def raw_projection(r, i, j, orc):
    """Sensor j's vertices in sensor i before the conversions to int: (x + 0.5, y + 0.5 as float64, tz as float32), in the reference's
    float32 arithmetic (color_ref.project's, which the agreement tests hold to color_ref_py's)."""
    from tests import color_ref
    d, po = frames(r), [0] + np.cumsum(r.widths.astype(np.int64) * r.heights).tolist()
    rgb = r.depth_colors[3 * po[j]:3 * po[j + 1]].reshape(d[j].shape + (3,))
    v = orc.create_vertices(d[j], rgb, r.intr[7 * j:7 * j + 7], r.wt[12 * j:12 * j + 12], r.bounds)
    R, t = color_ref._inverse(r.wt[12 * i:12 * i + 12])
    f32 = np.float32
    X, Y, Z = v["X"].astype(f32), v["Y"].astype(f32), v["Z"].astype(f32)
    tx = (X * R[0, 0] + Y * R[0, 1] + Z * R[0, 2]) + t[0]
    ty = (X * R[1, 0] + Y * R[1, 1] + Z * R[1, 2]) + t[1]
    tz = (X * R[2, 0] + Y * R[2, 1] + Z * R[2, 2]) + t[2]
    cx, cy, fx, fy = (f32(q) for q in r.intr[7 * i:7 * i + 4])
    with np.errstate(all="ignore"):
        return ((tx * fx) / tz + cx).astype(np.float64) + 0.5, (cy - (ty * fy) / tz).astype(np.float64) + 0.5, tz
