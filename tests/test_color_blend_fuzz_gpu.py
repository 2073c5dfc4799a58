"""Seeded fuzz of the colour blend: random ring rigs (tests/support.py: 1 - 8 sensors, ragged sizes from 1 x 1 up to about 96 x 80 or
one size for all, poses on rings of different density, crop boxes, sensors moved out of each other's view), here and there an empty or
an inverted crop box, 1 - 3 ticks in one plan, depth_tol in 1 .. 40 and min_confidence in 0 .. 21, through DeviceFusion.color_blend,
bit for bit against the definition (tests/color_blend_ref.py): vertex bytes and counters.  The default run covers
$LSN_BLEND_FUZZ_CASES cases (default 24); a scale run raises it."""
import os

import numpy as np
import pytest

from livescan3d_amd import synth
from tests import color_blend_ref as ref, support

pytestmark = pytest.mark.gpu

N_CASES = int(os.environ.get("LSN_BLEND_FUZZ_CASES", "24"))
SEED = int(os.environ.get("LSN_BLEND_FUZZ_SEED", "20261021"))
SIZES = support.ragged_or_equal(97, 81, [32, 64, 96], [24, 48, 80])


def _later_tick(rng, rig):
    """The rig's frames seen a moment later (same sizes, same calibration): some pixels lost, others a few millimetres off, new colours."""
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2").astype(np.int64)
    dm = np.where(rng.random(dm.shape) < 0.05, 0, np.where(dm > 0, np.clip(dm + rng.integers(-3, 4, dm.shape), 1, 65535), 0))
    dc = np.clip(rig.depth_colors.astype(np.int64) + rng.integers(-40, 41, rig.depth_colors.shape), 0, 255)
    depths, rgbs, po = [], [], 0
    for w, h in zip(rig.widths.tolist(), rig.heights.tolist()):
        depths.append(dm[po:po + w * h].reshape(h, w))
        rgbs.append(dc[3 * po:3 * (po + w * h)].reshape(h, w, 3))
        po += w * h
    return synth.Rig(depths, rgbs, rig.intr, rig.wt, rig.bounds)


def fuzz_case(case):
    rng = np.random.default_rng([SEED, case])
    rig = support.ring_rig(rng, 8, [6, 8, 12], SIZES)
    box = rng.random()
    if box < 0.08:      # empty: nothing survives
        rig.bounds = np.float32([5, 5, 5, 6, 6, 6])
    elif box < 0.16:    # inverted on one axis
        rig.bounds = rig.bounds.copy()
        rig.bounds[[0, 3]] = rig.bounds[[3, 0]]
    ticks = [rig]
    for _ in range(int(rng.integers(0, 3))):
        ticks.append(_later_tick(rng, ticks[-1]))
    return ticks, int(rng.integers(1, 41)), int(rng.integers(0, 22))


@pytest.mark.parametrize("case", range(N_CASES))
def test_color_blend_fuzz(gpu, orc, case):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    ticks, tol, minc = fuzz_case(case)
    what = (case, ticks[0].widths.tolist(), ticks[0].heights.tolist(), len(ticks), tol, minc)
    with DeviceFusion.from_rigs(ticks) as fus:
        fus.run()
        fus.color_blend(tol, minc)
        torch.cuda.synchronize()
        for k, rig in enumerate(ticks):
            want, diag = ref.blend(rig, orc, tol, minc)
            got, off = fus.tick_cloud(k)
            assert got.tobytes() == want.tobytes(), (what, k, len(got), len(want))
            d = fus.color_blend_diagnostics(k)
            assert all(np.array_equal(d[key], diag[key]) for key in diag), (what, k, {key: d[key].tolist() for key in diag}, {key: v.tolist() for key, v in diag.items()})
