"""Inputs of the export fixtures (test infrastructure): tests/golden/make_export_golden.py runs the reference's own exports on them,
tests/test_export_pin.py and tests/test_export_pin_gpu.py hold the oracle, the restatements and the GPU to what it wrote.

Every builder is a pure function of its arguments.  A case is (name, kind, rig, flag pairs):
  kind "mesh"        generateMeshFromDepthMaps with every (bcolor_transfer, bgenerate_triangles) pair listed, and
                     generateVerticesFromDepthMap for every index;
  kind "radial"      depthMapAndColorSetRadialCorrection;
  kind "radial_mesh" depthMapAndColorSetRadialCorrection, then generateMeshFromDepthMaps(false, false) and generateVerticesFromDepthMap
                     on the corrected frames (what lsnCorrectAndGenerateMesh and lsnTickRun compute).
SMALL cases keep their inputs and full outputs in tests/golden/export_ref.npz; large_cases() keep sha256 digests in
tests/golden/export_ref_digests.json.  The d_faces_* fixtures have box faces taken from the reference's own vertices
(crop_probe_cases, make_export_golden.py's first pass), so they are rebuilt from the fixture's stored inputs."""
import hashlib
import os

import numpy as np

from livescan3d_amd import synth
from tests import color_cases, color_ref, merge_cases

FF, ALL_FLAGS = [(0, 0)], [(0, 0), (1, 0), (0, 1), (1, 1)]
WIDE = np.array([-100, -100, -100, 100, 100, 100], dtype=np.float32)
IDENTITY_WT = synth.pack_pose(np.eye(3), np.zeros(3))
NAN, INF = float("nan"), float("inf")


def rig1(depth, rgb, intr, wt, bounds):
    return synth.Rig([depth], [rgb], intr, wt, bounds)


def noise_rig(sizes, seed, bounds=WIDE, intr=None, poses=None, depth_fn=None):
    """Noise frames of the given (w, h) sizes on ring poses; intr / poses override per sensor; depth_fn(depth, s) -> depth."""
    depths, rgbs, ii, ww = [], [], [], []
    for s, (w, h) in enumerate(sizes):
        d, c = synth.noise_frame(seed, 0, s, w, h)
        depths.append(depth_fn(d, s) if depth_fn else d)
        rgbs.append(c)
        ii.append(synth.kinect_intrinsics(w, h) if intr is None else np.asarray(intr[s], np.float32))
        ww.append(synth.pack_pose(*synth.ring_pose(s, max(len(sizes), 2))) if poses is None else np.asarray(poses[s], np.float32))
    return synth.Rig(depths, rgbs, np.concatenate(ii), np.concatenate(ww), bounds)


def _intr(w, h, **kw):
    p = synth.kinect_intrinsics(w, h).copy()
    for k, v in kw.items():
        p["cx cy fx fy r2 r4 r6".split().index(k)] = v
    return p


def _extremes(d, s):
    """Depth 1 and 65535 beside ordinary depths and holes."""
    rng = np.random.default_rng(100 + s)
    pick = rng.integers(0, 4, d.shape)
    return np.select([pick == 0, pick == 1, pick == 2], [np.uint16(1), np.uint16(65535), np.uint16(0)], d).astype(np.uint16)


def _levels(d, s):
    """Four depth levels only, so that many vertices share each coordinate value (and so sit exactly on a face of a box taken from them)."""
    return np.array([0, 1000, 1250, 1500, 2000], np.uint16)[(d.astype(np.int64) * 7 + s) % 5]


def depth_cases():
    """depth -> cloud: generateMeshFromDepthMaps(false, false) and generateVerticesFromDepthMap."""
    c = []
    one = np.full((1, 1), 1500, np.uint16), np.array([[[10, 20, 30]]], np.uint8)
    c.append(("d_1x1", "mesh", rig1(*one, _intr(1, 1), synth.pack_pose(*synth.ring_pose(0, 1)), WIDE), FF))
    c.append(("d_1x1_hole", "mesh", rig1(np.zeros((1, 1), np.uint16), one[1], _intr(1, 1), IDENTITY_WT, WIDE), FF))
    c.append(("d_1xN", "mesh", noise_rig([(37, 1)], 1), FF))
    c.append(("d_Nx1", "mesh", noise_rig([(1, 29)], 2), FF))
    c.append(("d_17x9_x2", "mesh", noise_rig([(17, 9)] * 2, 3, bounds=synth.DEFAULT_BOUNDS), FF))
    c.append(("d_513x3", "mesh", noise_rig([(513, 3)], 4, bounds=synth.DEFAULT_BOUNDS), FF))
    c.append(("d_extremes_wide", "mesh", noise_rig([(23, 11), (9, 7)], 5, depth_fn=_extremes), FF))
    c.append(("d_extremes_crop", "mesh", noise_rig([(23, 11), (9, 7)], 5, bounds=synth.DEFAULT_BOUNDS, depth_fn=_extremes), FF))
    c.append(("d_inverted_box", "mesh", noise_rig([(19, 13)], 6, bounds=np.float32([1, 1, 1, -1, -1, -1])), FF))
    c.append(("d_nan_box", "mesh", noise_rig([(19, 13)], 7, bounds=np.float32([NAN] * 6)), FF))
    c.append(("d_nan_faces", "mesh", noise_rig([(19, 13)], 8, bounds=np.float32([NAN, -0.2, NAN, 0.1, NAN, NAN])), FF))
    c.append(("d_inf_box", "mesh", noise_rig([(19, 13)], 9, bounds=np.float32([-INF, -INF, -INF, INF, INF, INF]),
                                              depth_fn=_extremes), FF))
    c.append(("d_inf_empty", "mesh", noise_rig([(19, 13)], 10, bounds=np.float32([INF, -INF, -INF, INF, INF, INF])), FF))
    c.append(("d_nan_fx", "mesh", noise_rig([(21, 9), (21, 9)], 11, bounds=synth.DEFAULT_BOUNDS,
                                             intr=[_intr(21, 9, fx=NAN), _intr(21, 9, fy=NAN)]), FF))
    c.append(("d_zero_fx", "mesh", noise_rig([(21, 9), (21, 9), (21, 9)], 12, bounds=synth.DEFAULT_BOUNDS,
                                              intr=[_intr(21, 9, fx=0.0, cx=10.0), _intr(21, 9, fy=0.0, cy=4.0),
                                                    _intr(21, 9, fx=0.0, fy=0.0, cx=3.0, cy=3.0)]), FF))
    c.append(("d_nan_pose", "mesh", noise_rig([(15, 10)], 13, bounds=synth.CROP_BOUNDS,
                                               poses=[np.float32([0, NAN, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1])]), FF))
    big = [synth.pack_pose(synth.rot_y(0.3), [1e6, -3e5, 2.5e4]), synth.pack_pose(synth.rot_y(-1.1), [-7e7, 1e-3, 4e8])]
    c.append(("d_big_translation", "mesh", noise_rig([(16, 12)] * 2, 14, bounds=np.float32([-1e9] * 3 + [1e9] * 3), poses=big), FF))
    c.append(("d_big_translation_crop", "mesh", noise_rig([(16, 12)] * 2, 14, bounds=np.float32([-2e6, -1e6, -1e6, 1e6, 1e6, 1e6]),
                                                           poses=big), FF))
    c.append(("d_mixed_sizes", "mesh", noise_rig([(17, 9), (24, 18), (1, 1), (33, 2), (8, 8)], 15, bounds=synth.DEFAULT_BOUNDS), FF))
    c.append(("d_n1", "mesh", synth.make_rig("scene", 1, 40, 34, seed=16), FF))
    c.append(("d_n8", "mesh", synth.make_rig("scene", 8, 24, 20, seed=17), FF))
    c.append(("d_n0", "mesh", synth.Rig([], [], np.zeros(0), np.zeros(0), synth.DEFAULT_BOUNDS), FF))
    return c


def crop_probe_cases():
    """Rigs whose box is cut from the reference's own vertices: the first pass runs them on WIDE, the fixture's box is then
    {min, max} of a quantile of each coordinate, so that many vertices sit exactly on a face."""
    return [("d_faces_identity", noise_rig([(31, 17)], 18, poses=[IDENTITY_WT], depth_fn=_levels)),
            ("d_faces_ring", noise_rig([(31, 17), (31, 17)], 19, depth_fn=_levels)),
            ("d_faces_scene", synth.make_rig("scene", 3, 32, 27, seed=20, bounds=WIDE))]


def _identity_intr(w, h, **kw):
    """cx = cy = 0, fx = fy = 1: with no distortion every pixel maps onto itself exactly."""
    p = np.float32([0, 0, 1, 1, 0, 0, 0])
    for k, v in kw.items():
        p["cx cy fx fy r2 r4 r6".split().index(k)] = v
    return p


def _neighbourhoods():
    """3 x 3 frames whose centre is a hole and whose 8 neighbours (raster order = the reference's shift order) test the prev_val rule
    (|v - prev_val| < 30: 29 counts, 30 does not; prev_val moves only when a neighbour counts) and n > 4 (4 does not close, 5 does)."""
    rng = np.random.default_rng(21)
    hand = [[1000] * 8, [1000, 1029, 1058, 1087, 1116, 1145, 1174, 1203], [1000, 1030, 1060, 1090, 1120, 1150, 1180, 1210],
            [1000, 1030, 1029, 971, 970, 1000, 1001, 0], [1000, 0, 1029, 0, 1000, 0, 1029, 0], [1000, 0, 1029, 0, 1000, 1058, 1029, 0],
            [1000, 0, 1029, 0, 1000, 1059, 1029, 1030], [0, 0, 0, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1, 0], [65535] * 8,
            [65535, 65506, 65535, 65506, 65535, 65477, 65506, 65535], [30, 1, 29, 58, 59, 0, 31, 2], [500, 529, 559, 530, 501, 471, 442, 470]]
    for _ in range(43):
        v = [int(rng.integers(1000, 1100))]
        for _ in range(7):
            v.append(0 if rng.random() < 0.15 else int(np.clip(v[-1] + rng.integers(-33, 34), 1, 65535)))
        hand.append(v)
    frames = []
    for v in hand:
        f = np.zeros((3, 3), np.uint16)
        f[0, 0], f[0, 1], f[0, 2], f[1, 0], f[1, 2], f[2, 0], f[2, 1], f[2, 2] = v
        frames.append(f)
    return frames


def _rgb(seed, w, h):
    return synth.noise_frame(seed, 1, 0, w, h)[1]


def _holes(w, h, seed, p, base=1500, spread=40):
    rng = np.random.default_rng(seed)
    d = np.clip(base + rng.integers(-spread, spread + 1, (h, w)), 1, 65535)
    return np.where(rng.random((h, w)) < p, 0, d).astype(np.uint16)


def _radial_rig(depths, intrs, seed=0):
    return synth.Rig(depths, [_rgb(seed + k, d.shape[1], d.shape[0]) for k, d in enumerate(depths)], np.concatenate(intrs),
                     np.concatenate([IDENTITY_WT] * len(depths)), WIDE)


def radial_cases():
    c = []
    tiny = [np.full((1, 1), 1200, np.uint16), np.full((2, 2), 1300, np.uint16), _holes(3, 3, 1, 0.3), np.zeros((3, 3), np.uint16)]
    c.append(("r_tiny_identity", "radial", _radial_rig(tiny, [_identity_intr(d.shape[1], d.shape[0]) for d in tiny]), FF))
    c.append(("r_tiny_kinect", "radial", _radial_rig(tiny, [synth.kinect_intrinsics(d.shape[1], d.shape[0]) for d in tiny], 1), FF))
    nb = _neighbourhoods()
    c.append(("r_prev_val", "radial", _radial_rig(nb, [_identity_intr(3, 3)] * len(nb), 2), FF))
    chains = [_holes(24, 18, 3, 0.45), _holes(24, 18, 4, 0.6, spread=20), _holes(31, 7, 5, 0.5, spread=14)]
    c.append(("r_hole_chains", "radial", _radial_rig(chains, [_identity_intr(d.shape[1], d.shape[0]) for d in chains], 3), FF))
    stair = np.full((12, 12), 2000, np.uint16)
    for k in range(1, 11):
        stair[k, k:] = 0        # a staircase of holes: every closed pixel is a neighbour of the next one in raster order
    c.append(("r_staircase", "radial", _radial_rig([stair, stair.T.copy()], [_identity_intr(12, 12)] * 2, 4), FF))
    k = [_holes(33, 21, 7, 0.25), _holes(17, 9, 8, 0.1)]
    c.append(("r_kinect_small", "radial", _radial_rig(k, [synth.kinect_intrinsics(d.shape[1], d.shape[0]) for d in k], 5), FF))
    w, h = 17, 13
    fold = [_intr(w, h, r2=3.0, r4=0, r6=0), _intr(w, h, r2=-40.0), _intr(w, h, r2=1e12), _intr(w, h, r2=-1e12, r4=1e20),
            _intr(w, h, r6=-1e30), _intr(w, h, fx=1e-30, fy=1e-30)]
    c.append(("r_fold_overflow", "radial", _radial_rig([_holes(w, h, 9 + q, 0.1) for q in range(len(fold))], fold, 6), FF))
    nans = [_intr(w, h, r2=NAN), _intr(w, h, cx=NAN), _intr(w, h, fy=NAN), _intr(w, h, fx=0.0, cx=14.0), _intr(w, h, r4=INF)]
    c.append(("r_nan_params", "radial", _radial_rig([_holes(w, h, 20 + q, 0.1) for q in range(len(nans))], nans, 7), FF))
    c.append(("r_scene_small", "radial", synth.make_rig("scene", 2, 32, 27, seed=22), FF))
    rm = synth.make_rig("scene", 3, 32, 27, seed=23)
    c.append(("rm_scene", "radial_mesh", rm, FF))
    rm2 = noise_rig([(17, 9), (24, 18), (1, 1), (2, 2), (3, 3)], 24, bounds=synth.DEFAULT_BOUNDS,
                    intr=[_intr(17, 9), _intr(24, 18, r2=-0.6), _intr(1, 1), _intr(2, 2), _intr(3, 3)])
    c.append(("rm_mixed", "radial_mesh", rm2, FF))
    return c


def colour_merge_cases():
    """Colour transfer and the overlay merge (every flag pair, equal sizes: the merge's defined case) on small frames."""
    c = []
    c.append(("cm_wall3", "mesh", merge_cases.wall(3, 32, 27), ALL_FLAGS))
    return c


SMALL = depth_cases() + radial_cases() + colour_merge_cases()


def large_cases():
    """Digest-only cases (rebuilt on every run)."""
    c = []
    for kind, n, w, h, seed in (("scene", 8, 512, 424, 3), ("noise", 8, 512, 424, 3), ("noise", 2, 1024, 1024, 3)):
        c.append((f"L_{kind}_{n}x{w}x{h}", "mesh", synth.make_rig(kind, n, w, h, seed=seed), FF))
    c.append(("L_radial_scene_8x512x424", "radial", synth.make_rig("scene", 8, 512, 424, seed=3), FF))
    big = synth.make_rig("noise", 2, 1024, 1024, seed=4)
    c.append(("L_radial_noise_2x1024x1024", "radial", big, FF))
    c.append(("L_radial_mesh_scene_8x512x424", "radial_mesh", synth.make_rig("scene", 8, 512, 424, seed=5), FF))
    for n in range(2, 9):
        c.append((f"L_ring{n}", "mesh", color_cases.ring(n, sizes=[(256, 212)] * n, of=8 if n < 8 else None), ALL_FLAGS))
    c.append(("L_ring8_full", "mesh", color_cases.ring(8), ALL_FLAGS))
    for n in (2, 3, 4):
        c.append((f"L_wall{n}", "mesh", merge_cases.wall(n), ALL_FLAGS))
    c.append(("L_twins", "mesh", merge_cases.twins(), ALL_FLAGS))
    c.append(("L_no_overlap", "mesh", color_cases.no_overlap(), ALL_FLAGS))
    c.append(("L_disjoint_pairs", "mesh", color_cases.disjoint_pairs(), ALL_FLAGS))
    c.append(("L_constant_colour", "mesh", color_cases.constant_colour(color_ref), ALL_FLAGS))
    for t in range(16):      # a 16-tick-like sequence of distinct rigs: the ring scene at successive ticks, four sensors
        c.append((f"L_seq_t{t:02d}", "mesh", color_cases.ring(4, sizes=[(128, 106)] * 4, of=8, tick=t, seed=30), [(1, 1)]))
    return c


# ---- fixture access (tests/test_export_pin.py, tests/test_export_pin_gpu.py) -----------------------------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def rig_inputs(rig):
    """Every input of a call, as the digests hash them."""
    return np.concatenate([rig.depth_maps.view(np.uint8), rig.depth_colors, rig.intr.view(np.uint8), rig.wt.view(np.uint8),
                           rig.bounds.view(np.uint8), rig.widths.view(np.uint8), rig.heights.view(np.uint8)])


def split(rig, depth_u8=None, colors=None):
    """[(depth (h, w) u16, rgb (h, w, 3) u8)] per sensor of the rig (or of the given buffers laid out as the rig's)."""
    dm = np.ascontiguousarray(rig.depth_maps if depth_u8 is None else depth_u8).view("<u2")
    dc = rig.depth_colors if colors is None else np.asarray(colors)
    out, po = [], 0
    for w, h in zip(rig.widths.tolist(), rig.heights.tolist()):
        out.append((dm[po:po + w * h].reshape(h, w), dc[3 * po:3 * (po + w * h)].reshape(h, w, 3)))
        po += w * h
    return out


def corrected_rig(rig, depth_u8, colors):
    """The rig with its frames replaced by radial correction's output."""
    f = split(rig, depth_u8, colors)
    return synth.Rig([d for d, _ in f], [c for _, c in f], rig.intr, rig.wt, rig.bounds)


def fixture_rig(z, name):
    """The synth.Rig a case of export_ref.npz was generated from (its stored inputs)."""
    p = name + "/"
    r = synth.Rig([np.zeros((h, w), np.uint16) for w, h in zip(z[p + "widths"].tolist(), z[p + "heights"].tolist())],
                  [np.zeros((h, w, 3), np.uint8) for w, h in zip(z[p + "widths"].tolist(), z[p + "heights"].tolist())],
                  z[p + "intr"], z[p + "wt"], z[p + "bounds"])
    return corrected_rig(r, z[p + "depth"].view(np.uint8), z[p + "colors"]) if r.n else r
