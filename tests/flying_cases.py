"""Frames and settings of the flying-pixel filter's fixture (test infrastructure): what tests/golden/make_flying_golden.py feeds the
reference's filterFlyingPixels, and the rigs the GPU tests run through the library.  Sizes are (w, h)."""
import numpy as np

from livescan3d_amd import synth
from tests import color_cases

RADII = (1, 2, 3, 7)
THRESHOLDS = (-1, 0, 1, 20, 65534, 65535, 70000)
THIRD_ARGUMENTS = (0, 4, 1000)   # the reference overwrites it: every case runs with all three and must give the same map
DIGEST_SIZES = ((512, 424), (1024, 1024))


def _rand(rng, w, h, lo=0, hi=65536):
    return rng.integers(lo, hi, (h, w)).astype(np.uint16)


def small_frames():
    """name -> u16 [h, w].  Patterns that land exactly on the strict comparisons, the sizes around 2r + 1, synthetic sensor frames."""
    rng = np.random.default_rng(20261017)
    f = {}
    # sizes 1x1 .. 513x9 with arbitrary values; 4x4, 8x6 and 16x16 so that 2r+1 is ONE BELOW a side for r = 1, 2 / 3, 7
    for w, h in ((1, 1), (2, 2), (3, 3), (3, 7), (4, 4), (8, 6), (16, 16), (17, 5), (513, 9)):
        f[f"random_{w}x{h}"] = _rand(rng, w, h, 900, 1100)
    f["wide_values_37x29"] = _rand(rng, 37, 29)
    # a straight step edge (an edge pixel: 3 of 8 differ, kept) and the corner of a quadrant (5 of 8: removed)
    y, x = np.mgrid[0:5, 0:17]
    f["step_edge_17x5"] = np.where(x < 8, 1000, 1100).astype(np.uint16)
    f["step_corner_17x5"] = np.where((x >= 8) & (y >= 2), 1100, 1000).astype(np.uint16)
    y, x = np.mgrid[0:29, 0:37]
    f["step_corner_37x29"] = np.where((x >= 18) & (y >= 14), 1100, 1000).astype(np.uint16)
    # checkerboard: the 4 edge neighbours differ, the 4 diagonal ones do not (4 of 8: kept)
    f["checkerboard_37x29"] = np.where((x + y) % 2 == 0, 1000, 1100).astype(np.uint16)
    # one-pixel lines and isolated pixels
    lines = np.full((29, 37), 1000, np.uint16)
    lines[:, 9] = 2000
    lines[20, :] = 2000
    lines[5, 20] = lines[12, 30] = lines[25, 3] = 3000
    f["lines_and_dots_37x29"] = lines
    # differences of exactly thr and thr + 1 (thr = 20, 1, 0): isolated pixels and 2x2 blocks on a flat background
    ex = np.full((29, 37), 1000, np.uint16)
    for k, dv in enumerate((20, 21, 1, 2, -20, -21, -1, -2)):
        ex[3, 3 + 4 * k] = 1000 + dv
        ex[9:11, 3 + 4 * k:5 + 4 * k] = 1000 + dv
        ex[16:19, 3 + 4 * k] = 1000 + dv
    f["exact_thresholds_37x29"] = ex
    # depth 0 against 65535 (difference 65535: above thr = 65534, not above 65535)
    ext = np.zeros((29, 37), np.uint16)
    ext[4, 4] = ext[10, 10:12] = 65535
    ext[15:, 20:] = 65535
    ext[20, 25] = ext[24, 30:32] = 0
    ext[5, 30] = 65534
    f["zero_against_65535_37x29"] = ext
    # two levels at random: full of kept pixels with exactly N / 2 differing neighbours next to removed ones of their own level --
    # a pass that saw its own zeros would remove them too (decisions on the unmodified map)
    f["two_levels_37x29"] = np.where(rng.random((29, 37)) < 0.5, 1000, 1100).astype(np.uint16)
    f["two_levels_holes_37x29"] = np.where(rng.random((29, 37)) < 0.15, 0, f["two_levels_37x29"]).astype(np.uint16)
    f["all_zero_37x29"] = np.zeros((29, 37), np.uint16)
    f["all_zero_96x80"] = np.zeros((80, 96), np.uint16)
    # synthetic sensors
    f["scene_96x80"] = synth.scene_frame(1, 0, 0, 8, 96, 80)[0]
    f["scene_s3_96x80"] = synth.scene_frame(1, 0, 3, 8, 96, 80)[0]
    f["noise_96x80"] = synth.noise_frame(1, 0, 0, 96, 80)[0]
    f["scene_513x9"] = synth.scene_frame(1, 0, 1, 8, 513, 9)[0]
    ring = color_cases.ring(2, sizes=[(96, 80), (37, 29)], of=8)
    dm = ring.depth_maps.view("<u2")
    f["ring_s0_96x80"] = dm[:96 * 80].reshape(80, 96).copy()
    f["ring_s1_37x29"] = dm[96 * 80:].reshape(29, 37).copy()
    return f


def small_cases(frames):
    """[(frame name, r, thr)]: the full cross of RADII x THRESHOLDS on the frames up to 37 x 29, a cut of it on the 513 x 9 and 96 x 80 ones."""
    out = []
    for name, d in frames.items():
        if d.size <= 37 * 29:
            out += [(name, r, t) for r in RADII for t in THRESHOLDS]
        else:
            out += [(name, r, 20) for r in RADII] + [(name, 1, t) for t in THRESHOLDS if t != 20] + [(name, 2, 0), (name, 2, 1)]
    return out


def digest_frame(spec):
    """The u16 [h, w] frame a digest entry names: {"kind": "scene" | "noise", "seed", "tick", "sensor", "of", "w", "h"}."""
    if spec["kind"] == "scene":
        return synth.scene_frame(spec["seed"], spec["tick"], spec["sensor"], spec["of"], spec["w"], spec["h"])[0]
    return synth.noise_frame(spec["seed"], spec["tick"], spec["sensor"], spec["w"], spec["h"])[0]


def digest_cases():
    """[(frame spec, r, thr)] of the frames kept by digest: the 8 scene sensors of the seed-1 ring and a noise frame at 512 x 424, a
    scene and a noise frame at 1024 x 1024."""
    out = []
    specs = [dict(kind="scene", seed=1, tick=0, sensor=s, of=8, w=512, h=424) for s in range(8)]
    for sp in specs:
        out.append((sp, 1, 20))
    big = [specs[0], dict(kind="noise", seed=1, tick=0, sensor=0, of=8, w=512, h=424),
           dict(kind="scene", seed=1, tick=0, sensor=2, of=8, w=1024, h=1024), dict(kind="noise", seed=1, tick=0, sensor=1, of=8, w=1024, h=1024)]
    for sp in big:
        out += [(sp, r, 20) for r in RADII if not (r == 1 and sp is specs[0])] + [(sp, 1, 0), (sp, 1, 1), (sp, 2, 65535), (sp, 3, -1)]
    return out
