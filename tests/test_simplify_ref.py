"""The CPU restatement of the mesh level-of-detail stage (tests/simplify_ref.py): hand-made clouds for every rule of the definition, the
known answers on the 3 x 96x80 ring, idempotence, the switch-off values, and the names the feature adds.  No GPU."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, simplify_ref
from tests.simplify_cases import cases

NAMES = ("lsnFusionSimplify", "lsnFusionSimplifyDiagnostics", "lsnLastMeshTransferFrameLod", "lsnLastMeshPlyLod")
# cell -> vertices kept on color_cases.ring(3, sizes=[(96, 80)] * 3): 11 087 vertices, sensor blocks at 3814 / 7283
RING_KEPT = {1e-6: 11087, 0.02: 10437, 0.05: 5040, 0.2: 495, 100.0: 8}


def run(name):
    xyz, off, tri, toff, cell = cases()[name]
    v = simplify_ref.cloud(xyz)
    return v, simplify_ref.simplify(v, off, tri, toff, cell)


def test_two_vertices_in_one_cell():
    v, o = run("two_in_one_cell")
    assert o["remap"].tolist() == [0, 0, 1] and o["offsets"].tolist() == [0, 2] and o["cells"] == 2 and o["unclustered"] == 0
    assert o["vertices"].tobytes() == v[[0, 2]].tobytes()      # the representative's own 16 bytes: nothing is averaged


def test_negative_coordinates_floor():
    _, o = run("negative_coordinates")
    assert o["remap"].tolist() == [0, 1, 2, 2, 0] and o["cells"] == 3


def test_coordinates_on_a_cell_boundary():
    _, o = run("on_the_boundary")
    assert o["remap"].tolist() == [0, 0, 1, 2, 3, 4] and o["cells"] == 5


def test_unclustered_vertices_are_kept():
    v, o = run("unclustered")
    # NaN, inf and q >= 2^20 or q < -2^20 are cells of their own, two by two; q = 2^20 - 1 and q = -2^20 cluster
    assert o["remap"].tolist() == [0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 8, 9, 9, 10, 11]
    assert o["unclustered"] == 9 and o["cells"] == 12


def test_triangles_collapse_drop_and_duplicate():
    _, o = run("triangles")
    assert o["remap"].tolist() == [0, 0, 1, 2, 3]
    assert o["triangles"].tolist() == [[1, 2, 3], [0, 1, 2], [0, 1, 2], [3, 2, 1], [2, 3, 0]]      # the same triple twice: both kept
    assert o["tri_offsets"].tolist() == [0, 5] and o["dropped_triangles"] == 6


def test_a_cell_across_two_sensor_blocks():
    _, o = run("two_sensors")
    assert o["remap"].tolist() == [0, 1, 2, 1, 3, 0, 3]
    assert o["offsets"].tolist() == [0, 3, 3, 4, 4]             # the later block loses vertex 3; the last block vanishes
    assert o["triangles"].tolist() == [[0, 1, 2], [1, 2, 3], [1, 3, 2], [0, 3, 2]] and o["tri_offsets"].tolist() == [0, 1, 1, 3, 4]


@pytest.fixture(scope="module")
def ring_mesh(orc):
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    v, counts, t = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    off = np.concatenate([[0], np.cumsum(counts[:3])]).astype(np.int32)
    return v, off, t, np.array([0, len(t) // 3, len(t) // 2, len(t)], np.int32)


def test_known_answers_on_the_ring(ring_mesh):
    v, off, t, toff = ring_mesh
    assert off.tolist() == [0, 3814, 7283, 11087]
    for cell, kept in RING_KEPT.items():
        o = simplify_ref.simplify(v, off, t, toff, cell)
        assert o["cells"] == kept == len(o["vertices"]) == o["offsets"][-1], cell
        assert o["dropped_triangles"] == len(t) - len(o["triangles"]) and o["tri_offsets"][-1] == len(o["triangles"])
    assert simplify_ref.simplify(v, off, t, toff, 0.05)["offsets"].tolist() == [0, 1958, 3500, 5040]
    assert simplify_ref.simplify(v, off, None, None, 0.05)["offsets"].tolist() == [0, 1958, 3500, 5040]


def test_idempotent(ring_mesh):
    v, off, t, toff = ring_mesh
    for cell in list(RING_KEPT) + [np.inf, 1e-40]:
        o = simplify_ref.simplify(v, off, t, toff, cell)
        again = simplify_ref.simplify(o["vertices"], o["offsets"], o["triangles"], o["tri_offsets"], cell)
        assert again["vertices"].tobytes() == o["vertices"].tobytes(), cell
        for k in ("offsets", "triangles", "tri_offsets"):
            assert np.array_equal(again[k], o[k]), (cell, k)
        assert again["remap"].tolist() == list(range(o["cells"]))


def test_infinite_and_denormal_cells_follow_the_arithmetic(ring_mesh):
    v, off, t, toff = ring_mesh
    one = simplify_ref.simplify(v, off, t, toff, np.inf)          # inv = 0: everything finite in one cell
    assert one["cells"] == 1 and len(one["triangles"]) == 0 and one["offsets"].tolist() == [0, 1, 1, 1]
    none = simplify_ref.simplify(v, off, t, toff, 1e-40)          # inv = inf: everything unclustered
    assert none["cells"] == none["unclustered"] == len(v) and np.array_equal(none["triangles"], t)


@pytest.mark.parametrize("cell", [0.0, -1.0, np.nan, -np.inf])
def test_switch_off_is_the_identity(ring_mesh, cell):
    v, off, t, toff = ring_mesh
    bad = np.concatenate([t[:10], [[0, 0, 0], [-1, 2, len(v)]], t[10:]]).astype(np.int32)      # copied as they are
    toff = toff + np.array([0, 2, 2, 2], np.int32)
    o = simplify_ref.simplify(v, off, bad, toff, cell)
    assert o["vertices"].tobytes() == v.tobytes() and np.array_equal(o["triangles"], bad)
    assert np.array_equal(o["offsets"], off) and np.array_equal(o["tri_offsets"], toff)
    assert o["remap"].tolist() == list(range(len(v))) and o["dropped_triangles"] == 0


def test_counts_are_clipped_and_negative_counts_are_zero():
    xyz, off, tri, toff, cell = cases()["triangles"]
    v = simplify_ref.cloud(xyz)
    o = simplify_ref.simplify(v, [0, 9], tri, [0, 99], cell, vertex_capacity=4, triangle_capacity=5)
    assert o["remap"].tolist() == [0, 0, 1, 2] and o["offsets"].tolist() == [0, 3]
    assert o["triangles"].tolist() == [[0, 1, 2], [0, 1, 2]] and o["tri_offsets"].tolist() == [0, 2] and o["dropped_triangles"] == 3
    o = simplify_ref.simplify(v, [0, -3], tri, [0, -1], cell)
    assert len(o["vertices"]) == 0 and len(o["triangles"]) == 0 and o["offsets"].tolist() == [0, 0] and o["tri_offsets"].tolist() == [0, 0]


def test_the_feature_is_declared():
    """Fails on a tree without the feature."""
    for name in NAMES:
        assert name in native.EXPORTS, name
    assert callable(getattr(native.FusionPlan, "simplify", None)) and callable(getattr(native.FusionPlan, "simplify_diagnostics", None))
    assert callable(getattr(native, "last_mesh_transfer_frame_lod", None)) and callable(getattr(native, "last_mesh_ply_lod", None))
