"""What only the tests need and several of them share: the seeded ring-rig fuzzer, the guard-band allocation, the merge export with its
error message, the child-process runner.  (The device batch itself is livescan3d_amd.fusion.DeviceFusion; torch is imported by the GPU
tests alone, so nothing here imports it.)"""
import os
import subprocess
import sys

import numpy as np

from livescan3d_amd import native, synth
from tests import color_cases, merge_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT_BOUNDS = np.array([-0.3, -1.0, -1.5, 1.5, 1.5, 1.5], dtype=np.float32)   # through the sphere, inside the views' overlap

GUARD = 4096
PATTERN = 0xA5


class Guarded:
    """`nbytes` of device memory with GUARD pattern bytes either side."""

    def __init__(self, torch, nbytes, dev):
        self.torch, self.n = torch, int(nbytes)
        self.buf = torch.full((GUARD + self.n + GUARD,), PATTERN, dtype=torch.uint8, device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.buf[:GUARD] == PATTERN).all().item()) and bool((self.buf[GUARD + self.n:] == PATTERN).all().item())


def export(rig, **flags):
    """generateMeshFromDepthMaps with native.generate_mesh_from_depth_maps' flags.  Returns (vertices, triangles, last error message)."""
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, **flags)
    return v, t, native.last_error()


def child(code, env_extra, *args, drop=(), timeout=300):
    """`code` (with sys.argv[1:] = args) in a fresh Python process started in the repository root, its environment this one's without the
    variables of `drop` and with env_extra.  It must exit with 0.  Returns (last line of its stdout, its stderr)."""
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code, *map(str, args)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1], r.stderr


def ragged_or_equal(max_w, max_h, widths, heights):
    """sizes(rng, n) for ring_rig: in half of the cases every sensor its own size below (max_w, max_h), else one size out of widths x heights."""
    def sizes(rng, n):
        if rng.random() < 0.5:
            return [(int(rng.integers(1, max_w)), int(rng.integers(1, max_h))) for _ in range(n)]
        w, h = int(rng.choice(widths)), int(rng.choice(heights))
        return [(w, h)] * n
    return sizes


def one_of(pairs):
    """sizes(rng, n) for ring_rig: one of `pairs` for all sensors."""
    return lambda rng, n: [pairs[int(rng.integers(0, len(pairs)))]] * n


def ring_rig(rng, max_n, densities, sizes, wall=None):
    """One random rig of the colour / outlier / merge fuzzers: 1..max_n sensors on a ring of n or one of `densities` positions, sizes(rng, n)
    their frame sizes, a random crop box in 70 % of the cases, every sensor moved out of the others' view with probability 0.15.
    wall = None: the density is drawn before the sizes.  wall = p: the sizes come first and with probability p the rig is a
    merge_cases.wall of the first size instead.  (The order of the draws is part of the fuzzers' cases: a seed names the same rig as ever.)"""
    n = int(rng.integers(1, max_n + 1))
    if wall is None:
        of = max(n, int(rng.choice([n] + densities)))
        sz = sizes(rng, n)
    else:
        sz = sizes(rng, n)
        if rng.random() < wall:
            return merge_cases.wall(n, *sz[0], seed=int(rng.integers(1, 1000)), step_deg=float(rng.uniform(0.0, 10.0)), tick=int(rng.integers(0, 5)))
        of = max(n, int(rng.choice([n] + densities)))
    lo, hi = rng.uniform(-1.6, -0.2, 3), rng.uniform(0.2, 1.6, 3)
    bounds = np.concatenate([lo, hi]).astype(np.float32) if rng.random() < 0.7 else color_cases.WIDE_BOUNDS
    poses = []
    for s in range(n):
        R, t = synth.ring_pose(s, of)
        if rng.random() < 0.15:   # this sensor's world is elsewhere
            t = t + R.T @ np.array([float(rng.uniform(5, 50)), 0.0, 0.0])
        poses.append((R, t))
    return color_cases.ring(n, sizes=sz, bounds=bounds, seed=int(rng.integers(1, 1000)), tick=int(rng.integers(0, 5)), poses=poses, of=of)
