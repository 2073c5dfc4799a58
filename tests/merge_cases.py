"""Rigs for the overlay-merge tests (test infrastructure): sensors facing one wall from nearby poses (large overlap with high
confidence, so the merge assigns many vertices), the same sensor twice (every mapped depth ties with the base's), and equal-sized
tiny frames.  The ring scene, the crop box and the non-overlapping pair come from tests/color_cases.py."""
import math

import numpy as np

from livescan3d_amd import synth

WIDE_BOUNDS = np.array([-100, -100, -100, 100, 100, 100], dtype=np.float32)


def wall_frame(R, t, w, h, seed, sensor, wall_z=0.0):
    """Ray-cast of the plane z = wall_z (a bump in the middle) from the camera of pose (R, t) (world p = R (p_cam + t)): depth u16, rgb."""
    intr = synth.kinect_intrinsics(w, h).astype(np.float64)
    cx, cy, fx, fy = intr[:4]
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack([(x - cx) / fx, (cy - y) / fy, np.ones_like(x)], axis=-1)
    o = R @ t
    d = dc @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (wall_z - o[2]) / d[..., 2]
    p = o + z[..., None] * d
    z = z - 0.2 * np.exp(-((p[..., 0] ** 2 + p[..., 1] ** 2) / 0.08))   # a smooth bump towards the cameras
    rng = np.random.default_rng(seed * 100 + sensor)
    depth = np.where(np.isfinite(z) & (z > 0.5) & (z < 4.5), np.rint(1000 * np.nan_to_num(z)), 0).astype(np.int64)
    depth = np.where(rng.random(depth.shape) < 0.01, 0, depth).astype(np.uint16)
    rgb = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    return depth, rgb


def wall(n=4, w=128, h=106, seed=1, step_deg=4.0, tick=0):
    """n sensors 1.5 m from the wall, turned by step_deg about y from one another."""
    depths, rgbs, intr, wt = [], [], [], []
    for s in range(n):
        R = synth.rot_y(math.radians(step_deg * (s - (n - 1) / 2) + 0.3 * tick))
        t = np.array([0.02 * s, 0.0, -1.5])
        d, c = wall_frame(R, t, w, h, seed + tick, s)
        depths.append(d)
        rgbs.append(c)
        intr.append(synth.kinect_intrinsics(w, h))
        wt.append(synth.pack_pose(R, t))
    return synth.Rig(depths, rgbs, np.concatenate(intr), np.concatenate(wt), WIDE_BOUNDS)


def twins(w=128, h=106):
    """The same sensor twice, then a third nearby one: sensor 1's mapped depths equal sensor 0's (ties everywhere)."""
    r = wall(2, w, h)
    dm = r.depth_maps.view("<u2").reshape(2, h, w)
    rgb = r.depth_colors.reshape(2, h, w, 3)
    three = wall(3, w, h, step_deg=3.0)
    d3 = three.depth_maps.view("<u2").reshape(3, h, w)
    return synth.Rig([dm[0], dm[0], d3[2]], [rgb[0], rgb[1], three.depth_colors.reshape(3, h, w, 3)[2]],
                     np.concatenate([r.intr[:7], r.intr[:7], three.intr[14:21]]), np.concatenate([r.wt[:12], r.wt[:12], three.wt[24:36]]),
                     WIDE_BOUNDS)
