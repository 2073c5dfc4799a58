"""Rigs for the colour-transfer tests (test infrastructure): the ring scene of livescan3d_amd/synth.py with a different colour gain and
offset per sensor (each Kinect's auto-exposure), and the edge rigs -- ragged sizes, disjoint pairs, views that do not overlap, a crop
box through the overlap, a constant-colour sensor, 1 x 1 and odd-sized frames, the shift_x frames of the confidence map."""
import numpy as np

from livescan3d_amd import synth

WIDE_BOUNDS = np.array([-100, -100, -100, 100, 100, 100], dtype=np.float32)


def _gain(rgb, sensor, seed):
    rng = np.random.default_rng(seed * 1000 + sensor)
    g = rng.uniform(0.7, 1.3, 3)
    o = rng.uniform(-25, 25, 3)
    return np.clip(np.rint(rgb.astype(np.float64) * g + o), 0, 255).astype(np.uint8)


def ring(n=8, sizes=None, bounds=None, seed=1, tick=0, gains=True, poses=None, of=None):
    """Scene frames of the first n sensors of an `of`-sensor ring (default of = n; synth.scene_frame / ring_pose); sizes: one (w, h)
    per sensor (default 512 x 424); poses: optional list of (R, t) replacing the world transforms handed to the call."""
    of = of or n
    sizes = sizes or [(512, 424)] * n
    depths, rgbs, intr, wt = [], [], [], []
    for s, (w, h) in enumerate(sizes):
        d, c = synth.scene_frame(seed, tick, s, of, w, h)
        depths.append(d)
        rgbs.append(_gain(c, s, seed) if gains else c)
        intr.append(synth.kinect_intrinsics(w, h))
        R, t = poses[s] if poses is not None else synth.ring_pose(s, of)
        wt.append(synth.pack_pose(R, t))
    return synth.Rig(depths, rgbs, np.concatenate(intr), np.concatenate(wt), synth.CROP_BOUNDS if bounds is None else bounds)


def _moved(sensor, n, dx):
    """ring_pose with the world moved by dx metres along x (p' = R (p + t): t += R^T [dx, 0, 0])."""
    R, t = synth.ring_pose(sensor, n)
    return R, t + R.T @ np.array([dx, 0.0, 0.0])


def disjoint_pairs(w=256, h=212):
    """Four sensors: 0 and 1 are ring neighbours, 2 and 3 the same two views with the world moved 50 m away.  The pairing takes
    (0, 1), finds no assigned map with an unassigned neighbour, and takes (2, 3) from its second branch."""
    poses = [synth.ring_pose(0, 8), synth.ring_pose(1, 8), _moved(0, 8, 50.0), _moved(1, 8, 50.0)]
    r = ring(8, sizes=[(w, h)] * 8, bounds=WIDE_BOUNDS)
    return _subset(r, [0, 1, 0, 1], poses, seed=3)


def no_overlap(w=256, h=212):
    """Two ring neighbours whose worlds are 50 m apart: no coverage, no change."""
    r = ring(8, sizes=[(w, h)] * 8, bounds=WIDE_BOUNDS)
    return _subset(r, [0, 1], [synth.ring_pose(0, 8), _moved(1, 8, 50.0)], seed=4)


def _subset(r, frames, poses, seed):
    sizes = list(zip(r.widths.tolist(), r.heights.tolist()))
    dm = r.depth_maps.view("<u2")
    starts = np.concatenate([[0], np.cumsum([w * h for w, h in sizes])])
    depths, rgbs, intr, wt = [], [], [], []
    for k, f in enumerate(frames):
        w, h = sizes[f]
        depths.append(dm[starts[f]:starts[f + 1]].reshape(h, w))
        rgbs.append(_gain(r.depth_colors[3 * starts[f]:3 * starts[f + 1]].reshape(h, w, 3), k, seed))
        intr.append(r.intr[7 * f:7 * f + 7])
        wt.append(synth.pack_pose(*poses[k]))
    return synth.Rig(depths, rgbs, np.concatenate(intr), np.concatenate(wt), r.bounds)


def constant_colour(color_ref, n=4, w=256, h=212, which=2):
    """A ring whose sensor `which` shows ONE colour wherever its confidence is >= 5 (so every transform sample of it has that colour and
    its deviation is 0: scale ~ 1e15) and its own colours on the low-confidence rim: those go out of int range and become 0."""
    r = ring(n, sizes=[(w, h)] * n, of=8)
    dm = r.depth_maps.view("<u2")
    start = which * w * h
    conf = color_ref.confidence_map(dm[start:start + w * h].reshape(h, w)).ravel()
    rgb = r.depth_colors[3 * start:3 * (start + w * h)].reshape(-1, 3)
    rgb[conf >= color_ref.MIN_CONFIDENCE] = (77, 140, 201)
    return r


def shift_x_frames(w=64, h=48):
    """Two depth frames whose confidence maps differ for an 8-neighbour wall test but not for the reference's, whose probes are
    (-1,-1), (0,0), (1,1) (depthprocessing.cpp:320): A is flat, B has a 300 mm step along the diagonal x - y = 10, which those probes
    never cross.  Returns (A, B) u16 (h, w)."""
    y, x = np.mgrid[0:h, 0:w]
    a = np.full((h, w), 1500, dtype=np.uint16)
    b = np.where(x - y < 10, 1500, 1800).astype(np.uint16)
    for f in (a, b):
        f[30:36, 20:26] = 0   # a hole: seeds around it and a BFS from them
    return a, b
