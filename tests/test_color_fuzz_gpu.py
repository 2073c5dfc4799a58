"""Seeded fuzz of the colour transfer: random rigs (sensor count, ragged and odd sizes, poses on rings of different density, crop boxes,
colour gains, sensors moved out of each other's view) through generateMeshFromDepthMaps(bcolor_transfer = true), bit-exact against the
CPU reference (tests/color_ref.py).  The default run covers $LSN_COLOR_FUZZ_CASES cases (default 12); a scale run raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_ref, support

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_COLOR_FUZZ_CASES", "12"))
SEED = int(os.environ.get("LSN_COLOR_FUZZ_SEED", "20261015"))
SIZES = support.ragged_or_equal(300, 260, [128, 256, 512], [106, 212, 424])


@pytest.mark.parametrize("case", range(N_CASES))
def test_color_transfer_fuzz(gpu, orc, case):
    rng = np.random.default_rng([SEED, case])
    rig = support.ring_rig(rng, 6, [6, 8, 12], SIZES)
    got, _ = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                  color_transfer=True)
    assert native.last_error() == ""
    want, diag = color_ref.color_transfer(rig, orc)
    assert got.tobytes() == want.tobytes(), (case, rig.widths.tolist(), rig.heights.tolist(), diag["pairs"])
