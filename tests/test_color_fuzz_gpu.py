"""Seeded fuzz of the colour transfer: random rigs (sensor count, ragged and odd sizes, poses on rings of different density, crop boxes,
colour gains, sensors moved out of each other's view) through generateMeshFromDepthMaps(bcolor_transfer = true), bit-exact against the
CPU reference (tests/color_ref.py).  The default run covers $LSN_COLOR_FUZZ_CASES cases (default 12); a scale run raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, color_ref

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_COLOR_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_COLOR_FUZZ_SEED", "20261015"))


def _rig(rng):
    n = int(rng.integers(1, 7))
    of = int(rng.choice([n, 6, 8, 12]))
    of = max(of, n)
    if rng.random() < 0.5:
        sizes = [(int(rng.integers(1, 300)), int(rng.integers(1, 260))) for _ in range(n)]
    else:
        w, h = int(rng.choice([128, 256, 512])), int(rng.choice([106, 212, 424]))
        sizes = [(w, h)] * n
    lo = rng.uniform(-1.6, -0.2, 3)
    hi = rng.uniform(0.2, 1.6, 3)
    bounds = np.concatenate([lo, hi]).astype(np.float32) if rng.random() < 0.7 else color_cases.WIDE_BOUNDS
    poses = []
    for s in range(n):
        R, t = synth.ring_pose(s, of)
        if rng.random() < 0.15:   # this sensor's world is elsewhere
            t = t + R.T @ np.array([float(rng.uniform(5, 50)), 0.0, 0.0])
        poses.append((R, t))
    return color_cases.ring(n, sizes=sizes, bounds=bounds, seed=int(rng.integers(1, 1000)), tick=int(rng.integers(0, 5)), poses=poses, of=of)


@pytest.mark.parametrize("case", range(N_CASES))
def test_color_transfer_fuzz(gpu, orc, case):
    rng = np.random.default_rng([SEED, case])
    rig = _rig(rng)
    got, _ = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                  color_transfer=True)
    assert native.last_error() == ""
    want, diag = color_ref.color_transfer(rig, orc)
    assert got.tobytes() == want.tobytes(), (case, rig.widths.tolist(), rig.heights.tolist(), diag["pairs"])
