"""The oracle's radial correction (oracle/lsn_oracle.c::orc_radial_correction) against an independent pure-Python /
numpy-float32 restatement of depthMapAndColorRadialCorrection (src/NativeUtils/depthprocessing.cpp:191-261).
Pinned: tests/test_export_pin.py holds both restatements to the reference's own depthMapAndColorSetRadialCorrection
(tests/golden/export_ref.npz, export_ref_digests.json); here the two must agree bit for bit on further frames."""
import numpy as np
import pytest

from livescan3d_amd import synth


def py_radial(depth2d, rgb3, intr):
    f = np.float32
    h, w = depth2d.shape
    cx, cy, fx, fy, r2, r4, r6 = [f(v) for v in intr]
    depth = depth2d.ravel()
    colors = rgb3.reshape(-1, 3)
    map_copy = np.zeros(w * h, np.uint16)
    colors_copy = np.zeros((w * h, 3), np.uint8)

    def f2i(v):
        if not (v > f(-2147483904.0) and v < f(2147483648.0)):   # NaN / out of range: cvttss2si -> INT_MIN
            return -2147483648
        return int(np.trunc(v))

    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if depth[x + y * w] == 0:
                    continue
                u = (f(x) - cx) / fx
                v = (f(y) - cy) / fy
                r = u * u + v * v
                d = f(1) - r2 * r - r4 * r * r - r6 * r * r * r
                xc = f2i(u * d * fx + cx)
                yc = f2i(v * d * fy + cy)
                if 0 <= xc < w and 0 <= yc < h:
                    map_copy[xc + yc * w] = depth[x + y * w]
                    colors_copy[xc + yc * w] = colors[x + y * w]
    shifts = [-w - 1, -w, -w + 1, -1, 1, w - 1, w, w + 1]
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            pos = x + y * w
            if map_copy[pos] != 0:
                continue
            n = s = 0
            sc = [0, 0, 0]
            prev = -1
            for sh in shifts:
                mv = int(map_copy[pos + sh])
                if mv > 0 and (prev == -1 or abs(mv - prev) < 30):
                    prev = mv
                    n += 1
                    s += mv
                    for c in range(3):
                        sc[c] += int(colors_copy[pos + sh, c])
            if n > 4:
                map_copy[pos] = s // n
                for c in range(3):
                    colors_copy[pos, c] = sc[c] // n
    return map_copy.reshape(h, w), colors_copy.reshape(h, w, 3)


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
