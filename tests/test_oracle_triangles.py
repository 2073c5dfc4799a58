"""The oracle's triangulation (oracle/lsn_oracle.c::orc_generate_triangles) against an independent pure-Python
restatement of MeshGenerator::generateTrianglesGradients (tests/tri_ref.py: src/NativeUtils/meshGenerator.cpp:14-181, including the
4-thread row-band split the reference uses, :147-181), on small frames -- and, the pin proper, against the REFERENCE's
own meshGenerator.cpp: committed fixtures made by tests/golden/make_tri_golden.py from oracle/_ref/libref_tri.so, plus
a wider live sweep (up to 512x424) whenever that compiled reference is present."""
import os

import numpy as np
import pytest

from livescan3d_amd import synth
from tests.tri_ref import py_triangles


@pytest.mark.parametrize("w,h", [(40, 30), (33, 21), (64, 9), (5, 5), (8, 4)])
def test_c_oracle_equals_python_restatement(orc, w, h):
    rng = np.random.default_rng(w * 100 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    for name, d in (("ramp", 1500 + 4 * xx + 3 * yy),
                    ("steps", 1500 + 4 * xx + 35 * ((xx // 5) % 2) + 28 * ((yy // 4) % 2)),
                    ("noise", 1500 + rng.integers(-14, 15, size=(h, w))),
                    ("holes", np.where(rng.random((h, w)) < 0.1, 0, 1400 + 9 * xx + 7 * yy))):
        depth = np.clip(d, 0, 65535).astype(np.uint16)
        rgb = synth.noise_frame(2, 0, 0, w, h)[1]
        intr, wt = synth.kinect_intrinsics(w, h), synth.pack_pose(*synth.ring_pose(0, 1))
        v, v2p, p2v = orc.create_vertices(depth, rgb, intr, wt, [-0.4, -5, -5, 0.5, 5, 5], want_maps=True)
        got = orc.generate_triangles(depth, p2v, index_base=7)
        want = py_triangles(depth, p2v)
        assert got.shape == want.shape, name
        assert np.array_equal(got, want + 7 if len(want) else want), name


def test_generate_mesh_rebases_indices_per_sensor(orc):
    rig = synth.make_rig("scene", 3, 96, 80, seed=5)
    v, counts, tri = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    v2, counts2 = orc.generate_mesh_vertices(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    assert v.tobytes() == v2.tobytes() and list(counts) == list(counts2)
    assert len(tri) > 0 and tri.min() >= 0 and tri.max() < len(v)
    # a triangle never mixes sensors (formMesh rebases each sensor's triangles by its own vertex offset, :1614-1626)
    edges = np.concatenate([[0], np.cumsum(counts)])
    sensor_of = np.searchsorted(edges, tri, side="right") - 1
    assert (sensor_of[:, 0] == sensor_of[:, 1]).all() and (sensor_of[:, 1] == sensor_of[:, 2]).all()
    assert (np.diff(sensor_of[:, 0]) >= 0).all()                         # sensor-major order


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_reference.npz")


def test_oracle_equals_reference_fixtures(orc):
    """tri_reference.npz holds the output of the reference's own generateTrianglesGradients."""
    z = np.load(GOLDEN)
    assert len(z["names"]) >= 20
    for name in z["names"]:
        depth, p2v, want = z[f"{name}_depth"], z[f"{name}_p2v"], z[f"{name}_tri"]
        got = orc.generate_triangles(depth, p2v)
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_oracle_equals_compiled_reference_sweep(orc):
    """Live comparison with oracle/_ref/libref_tri.so (src/NativeUtils/meshGenerator.cpp compiled as it lies)."""
    if not orc.have_ref_tri():
        pytest.skip("oracle/_ref/libref_tri.so not built (needs /root/reference)")
    rng = np.random.default_rng(77)
    total = 0
    for (w, h) in ((512, 424), (640, 576), (97, 61), (16, 16), (4, 4), (3, 9), (200, 5)):
        yy, xx = np.mgrid[0:h, 0:w]
        for k in range(4):
            base = rng.integers(300, 9000)
            d = base + rng.integers(1, 12) * xx + rng.integers(1, 9) * yy + rng.integers(-20, 21, size=(h, w)) * (k % 2) \
                + 60 * ((xx // rng.integers(3, 40)) % 2) * (k // 2)
            depth = np.clip(d, 0, 65535).astype(np.uint16)
            depth[rng.random((h, w)) < 0.04] = 0
            valid = (depth != 0) & ~(rng.random((h, w)) < 0.02)
            p2v = np.where(valid.ravel(), np.cumsum(valid.ravel()) - 1, -1).astype(np.int32)
            got, want = orc.generate_triangles(depth, p2v), orc.ref_triangles(depth, p2v)
            assert got.shape == want.shape and np.array_equal(got, want), (w, h, k)
            total += len(want)
    assert total > 500000
