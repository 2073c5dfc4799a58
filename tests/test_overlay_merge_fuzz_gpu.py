"""Seeded fuzz of the overlay merge: random rigs (sensor count, equal sizes from tiny to Kinect, ring density, wall rigs, crop boxes,
sensors moved out of each other's view) through generateMeshFromDepthMaps(bgenerate_triangles = true) with the merge switched on,
bit-exact against the CPU reference (tests/merge_ref.py).  The default run covers $LSN_MERGE_FUZZ_CASES cases (default 12); a scale run
raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, merge_cases, merge_ref

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_MERGE_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_MERGE_FUZZ_SEED", "20261015"))


def _rig(rng):
    n = int(rng.integers(1, 7))
    w, h = [(3, 3), (17, 13), (64, 53), (128, 106), (256, 212)][int(rng.integers(0, 5))]
    if rng.random() < 0.4:
        return merge_cases.wall(n, w, h, seed=int(rng.integers(1, 1000)), step_deg=float(rng.uniform(0.0, 10.0)), tick=int(rng.integers(0, 5)))
    of = max(n, int(rng.choice([n, 8, 16, 32])))
    lo, hi = rng.uniform(-1.6, -0.2, 3), rng.uniform(0.2, 1.6, 3)
    bounds = np.concatenate([lo, hi]).astype(np.float32) if rng.random() < 0.7 else color_cases.WIDE_BOUNDS
    poses = []
    for s in range(n):
        R, t = synth.ring_pose(s, of)
        if rng.random() < 0.15:   # this sensor's world is elsewhere
            t = t + R.T @ np.array([float(rng.uniform(5, 50)), 0.0, 0.0])
        poses.append((R, t))
    return color_cases.ring(n, sizes=[(w, h)] * n, bounds=bounds, seed=int(rng.integers(1, 1000)), tick=int(rng.integers(0, 5)), poses=poses,
                            of=of)


@pytest.mark.parametrize("case", range(N_CASES))
def test_overlay_merge_fuzz(gpu, orc, case):
    rng = np.random.default_rng([SEED, case])
    rig = _rig(rng)
    got, tris = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                     generate_triangles=True, overlay_merge=True)
    assert native.last_error() == ""
    want, diag = merge_ref.overlay_merge(rig, orc)
    assert np.array_equal(tris, want), (case, rig.n, rig.widths.tolist(), int(diag["assigned"].sum()))
