"""Seeded fuzz of the outlier filter: random rigs (sensor count, ragged and odd sizes, ring density, crop boxes, sensors moved away) and
random (k, maxDist) through generateVerticesFromDepthMap with the filter, bit-exact against filter() of the restatement (tests/outlier_ref.py)
on the unfiltered cloud.  The default run covers $LSN_OUTLIER_FUZZ_CASES cases (default 12); a scale run raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import outlier_ref, support

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_OUTLIER_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_OUTLIER_FUZZ_SEED", "20261016"))
SIZES = support.ragged_or_equal(200, 160, [64, 128, 256], [53, 106, 212])


@pytest.mark.parametrize("case", range(N_CASES))
def test_outlier_filter_fuzz(gpu, case):
    rng = np.random.default_rng([SEED, case])
    rig = support.ring_rig(rng, 4, [6, 8], SIZES)
    k = int(rng.choice([1, 2, 3, 5, 10, 20, 50]))
    d = float(rng.choice([0.002, 0.005, 0.01, 0.02, 0.05, 0.1, 0.3]))
    for i in range(rig.n):
        args = (rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
        plain = native.generate_vertices_from_depth_map(*args)
        got = native.generate_vertices_from_depth_map(*args, outlier_filter=(k, d))
        want = outlier_ref.filter_vertices(plain, k, d)
        assert got.tobytes() == want.tobytes(), (case, i, k, d, rig.widths.tolist(), rig.heights.tolist())
