"""Seeded fuzz of the outlier filter: random rigs (sensor count, ragged and odd sizes, ring density, crop boxes, sensors moved away) and
random (k, maxDist) through generateVerticesFromDepthMap with the filter, bit-exact against filter() of the restatement (tests/outlier_ref.py)
on the unfiltered cloud.  The default run covers $LSN_OUTLIER_FUZZ_CASES cases (default 12); a scale run raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, outlier_ref

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_OUTLIER_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_OUTLIER_FUZZ_SEED", "20261016"))


def _rig(rng):
    n = int(rng.integers(1, 5))
    of = max(n, int(rng.choice([n, 6, 8])))
    if rng.random() < 0.5:
        sizes = [(int(rng.integers(1, 200)), int(rng.integers(1, 160))) for _ in range(n)]
    else:
        w, h = int(rng.choice([64, 128, 256])), int(rng.choice([53, 106, 212]))
        sizes = [(w, h)] * n
    lo = rng.uniform(-1.6, -0.2, 3)
    hi = rng.uniform(0.2, 1.6, 3)
    bounds = np.concatenate([lo, hi]).astype(np.float32) if rng.random() < 0.7 else color_cases.WIDE_BOUNDS
    poses = []
    for s in range(n):
        R, t = synth.ring_pose(s, of)
        if rng.random() < 0.15:
            t = t + R.T @ np.array([float(rng.uniform(5, 50)), 0.0, 0.0])
        poses.append((R, t))
    return color_cases.ring(n, sizes=sizes, bounds=bounds, seed=int(rng.integers(1, 1000)), tick=int(rng.integers(0, 5)), poses=poses, of=of)


@pytest.mark.parametrize("case", range(N_CASES))
def test_outlier_filter_fuzz(gpu, case):
    rng = np.random.default_rng([SEED, case])
    rig = _rig(rng)
    k = int(rng.choice([1, 2, 3, 5, 10, 20, 50]))
    d = float(rng.choice([0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.3]))
    for i in range(rig.n):
        args = (rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
        plain = native.generate_vertices_from_depth_map(*args)
        got = native.generate_vertices_from_depth_map(*args, outlier_filter=(k, d))
        want = outlier_ref.filter_vertices(plain, k, d)
        assert got.tobytes() == want.tobytes(), (case, i, k, d, rig.widths.tolist(), rig.heights.tolist())
