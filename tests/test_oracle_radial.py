"""The oracle's radial correction (oracle/lsn_oracle.c::orc_radial_correction) against an independent pure-Python /
numpy-float32 restatement of depthMapAndColorRadialCorrection (src/NativeUtils/depthprocessing.cpp:191-261).
Pinned: tests/test_export_pin.py holds both restatements to the reference's own depthMapAndColorSetRadialCorrection
(tests/golden/export_ref.npz, export_ref_digests.json); here the two must agree bit for bit on further frames."""
import numpy as np
import pytest

from livescan3d_amd import synth
from tests.depth_ref import py_radial


@pytest.mark.parametrize("w,h,dist", [(40, 30, (0.09, -0.27, 0.09)), (33, 21, (0.5, 0.0, 0.0)), (24, 16, (0.0, 0.0, 0.0)),
                                      (16, 12, (float("nan"), 0.0, 0.0)), (20, 15, (-0.6, 0.2, 0.05))])
def test_c_oracle_equals_python_restatement(orc, w, h, dist):
    rng = np.random.default_rng(w + 7 * h)
    yy, xx = np.mgrid[0:h, 0:w]
    for name, d in (("ramp", 1500 + 5 * xx + 3 * yy), ("gaps", np.where((xx + 2 * yy) % 5 == 0, 0, 1500 + 5 * xx + 3 * yy)),
                    ("random", np.where(rng.random((h, w)) < 0.3, 0, 1500 + rng.integers(-40, 41, size=(h, w))))):
        depth = np.clip(d, 0, 65535).astype(np.uint16)
        rgb = synth.noise_frame(7, 0, 0, w, h)[1]
        intr = synth.kinect_intrinsics(w, h).copy()
        intr[4:7] = dist
        got_d, got_c = orc.radial_correction(depth, rgb, [w], [h], intr)
        want_d, want_c = py_radial(depth, rgb, intr)
        assert np.array_equal(got_d.view(np.uint16).reshape(h, w), want_d), name
        assert np.array_equal(got_c.reshape(h, w, 3), want_c), name


def test_all_sensors_and_threads(orc):
    rig = synth.make_rig("scene", 3, 96, 80, seed=2)
    a = orc.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, n_threads=1)
    b = orc.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, n_threads=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.array_equal(a[0], rig.depth_maps)
