"""Seeded fuzz of the overlay merge: random rigs (sensor count, equal sizes from tiny to Kinect, ring density, wall rigs, crop boxes,
sensors moved out of each other's view) through generateMeshFromDepthMaps(bgenerate_triangles = true) with the merge switched on,
bit-exact against the CPU reference (tests/merge_ref.py).  The default run covers $LSN_MERGE_FUZZ_CASES cases (default 12); a scale run
raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import merge_ref, support

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_MERGE_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_MERGE_FUZZ_SEED", "20261015"))
SIZES = support.one_of([(3, 3), (17, 13), (64, 53), (128, 106), (256, 212)])


@pytest.mark.parametrize("case", range(N_CASES))
def test_overlay_merge_fuzz(gpu, orc, case):
    rng = np.random.default_rng([SEED, case])
    rig = support.ring_rig(rng, 6, [8, 16, 32], SIZES, wall=0.4)
    got, tris = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                     generate_triangles=True, overlay_merge=True)
    assert native.last_error() == ""
    want, diag = merge_ref.overlay_merge(rig, orc)
    assert np.array_equal(tris, want), (case, rig.n, rig.widths.tolist(), int(diag["assigned"].sum()))
