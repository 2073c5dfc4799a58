"""generateMeshFromDepthMaps(bgenerate_triangles = true) with the overlay merge switched on, and lsnFusionOverlayMerge, on the GPU
against the CPU reference (tests/merge_ref.py).

Bar: bit-exact -- the triangles equal the reference's; the vertices are byte-identical to the call without the merge; the
diagnostics (reprojected maps, final maps, point_assigned) equal the reference's."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, color_ref, merge_cases, merge_ref
from tests.support import CUT_BOUNDS, ROOT, child, export

pytestmark = pytest.mark.gpu

MERGED = dict(generate_triangles=True, overlay_merge=True)
PLAIN = dict(overlay_merge=False)


def _device(rigs, order=("merge",)):
    """run_mesh over a batch of ticks, then the stages of `order` ("merge", "color"); synchronised."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    fus = DeviceFusion.from_rigs(rigs)
    fus.run_mesh()
    for stage in order:
        {"merge": fus.overlay_merge, "color": fus.color_transfer}[stage]()
    torch.cuda.synchronize()
    return fus


def _check_device(rig, orc, expect_assigned=None):
    fus = _device([rig])
    tris = fus.tick_triangles(0)
    want, diag = merge_ref.overlay_merge(rig, orc)
    assert tris.shape == want.shape and np.array_equal(tris, want), (tris.shape, want.shape)
    nv = int(fus.host_offsets()[0, -1])
    d = fus.plan.overlay_diagnostics(0, nv)
    assert np.array_equal(d["reprojected"], diag["reprojected"])
    assert np.array_equal(d["merged"], diag["merged"])
    assert np.array_equal(d["assigned"], diag["assigned"]) and d["n_assigned"] == int(diag["assigned"].sum())
    if expect_assigned is not None:
        assert (d["n_assigned"] > 0) == expect_assigned, d["n_assigned"]
    fus.close()
    return want, diag


def _check_export(rig, orc):
    plain, t0, e0 = export(rig, **PLAIN)
    got, t1, e1 = export(rig, **MERGED)
    want, _ = merge_ref.overlay_merge(rig, orc)
    assert e0 == "" and e1 == "", (e0, e1)
    assert got.tobytes() == plain.tobytes()                       # the merge touches no vertex
    assert np.array_equal(t1, want)
    return got, t1


def test_wall_export_is_merged(gpu, orc):
    """Fails without the feature: the flag used to be ignored (unmerged triangles, an error message)."""
    rig = merge_cases.wall(4)
    got, tris = _check_export(rig, orc)
    assert native.last_mesh_ply() == orc.ply_binary(got, tris)   # lsnLastMesh* serves the merged mesh
    _, plain_tris, _ = export(rig, **PLAIN)
    assert len(tris) < len(plain_tris)


def test_ring_4_and_8(gpu, orc):
    _check_device(color_cases.ring(4, sizes=[(256, 212)] * 4, of=32), orc, True)
    _check_device(color_cases.ring(8, sizes=[(256, 212)] * 8), orc)
    _check_export(color_cases.ring(8), orc)


def test_wall_8_device(gpu, orc):
    _check_device(merge_cases.wall(8, 256, 212), orc, True)


def test_one_sensor_is_the_reprojection(gpu, orc):
    rig = color_cases.ring(1, sizes=[(256, 212)], of=8)
    want, diag = _check_device(rig, orc, False)
    assert np.array_equal(diag["reprojected"], diag["merged"])
    # the triangles differ from the plain call only through the reprojection's rounding
    _, plain, _ = export(rig, **PLAIN)
    assert abs(len(want) - len(plain)) < 0.05 * len(plain)


def test_no_overlap(gpu, orc):
    _check_device(color_cases.no_overlap(), orc, False)


def test_crop_through_the_overlap(gpu, orc):
    _check_device(color_cases.ring(8, sizes=[(256, 212)] * 8, bounds=CUT_BOUNDS), orc)


def test_tiny_frames(gpu, orc):
    for size in ((1, 1), (3, 3), (7, 5), (37, 29)):
        _check_device(color_cases.ring(3, sizes=[size] * 3, of=8), orc)


def test_twins_depth_ties(gpu, orc):
    _check_device(merge_cases.twins(), orc, True)


def test_batch_equals_ticks_one_by_one(gpu, orc):
    T = 16
    rigs = [merge_cases.wall(4, 128, 106, tick=k) for k in range(T)]
    for r in rigs[1:]:   # one calibration for the plan
        r.intr, r.wt, r.bounds = rigs[0].intr, rigs[0].wt, rigs[0].bounds
    with _device(rigs) as fus:
        tris = [fus.tick_triangles(k) for k in range(T)]
    for k in range(T):
        with _device([rigs[k]]) as one:
            assert np.array_equal(tris[k], one.tick_triangles(0)), k
    want, _ = merge_ref.overlay_merge(rigs[5], orc)
    assert np.array_equal(tris[5], want)


def test_merge_and_colour_in_both_orders(gpu, orc):
    rig = merge_cases.wall(4)
    with _device([rig], ("merge", "color")) as f1, _device([rig], ("color", "merge")) as f2:
        v1, v2 = f1.vertices.cpu().numpy(), f2.vertices.cpu().numpy()
        t1, t2 = f1.tick_triangles(0), f2.tick_triangles(0)
    want, _ = merge_ref.overlay_merge(rig, orc)
    cwant, _ = color_ref.color_transfer(rig, orc)
    assert np.array_equal(t1, want) and np.array_equal(t2, want)
    assert v1.tobytes() == v2.tobytes() and v1[0, :len(cwant)].tobytes() == cwant.tobytes()
    got, tris, err = export(rig, color_transfer=True, **MERGED)
    assert err == "" and got.tobytes() == cwant.tobytes() and np.array_equal(tris, want)


def test_mixed_sizes_rejected(gpu):
    import torch
    rig = color_cases.ring(2, sizes=[(128, 106), (96, 80)], of=8)
    plan = native.FusionPlan(0, 1, rig.widths, rig.heights)
    plan.set_params(rig.intr, rig.wt, rig.bounds)
    cap = plan.capacity
    buf = torch.zeros(16 * cap + 24 * cap + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(native.NativeUtilsError, match="same size"):
        plan.overlay_merge(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 0)
    # the export: the unmerged mesh and a message
    plain, t0, _ = export(rig, generate_triangles=True, **PLAIN)
    got, t1, err = export(rig, **MERGED)
    assert "same size" in err and got.tobytes() == plain.tobytes() and np.array_equal(t0, t1)


def test_switch_off_behaves_as_before(gpu):
    rig = color_cases.ring(4, sizes=[(256, 212)] * 4, of=8)
    prev = native.set_overlay_merge(False)
    try:
        v0, t0, e0 = export(rig, generate_triangles=True)
        assert "overlay merge are outside this library's scope" in e0
        plain, tp, _ = export(rig)
        assert v0.tobytes() == plain.tobytes() and np.array_equal(t0, tp)
    finally:
        native.set_overlay_merge(prev)


def test_switch_is_restored_and_silent(gpu, capfd):
    prev = native.set_overlay_merge(False)
    try:
        export(merge_cases.wall(2), **MERGED)
        assert native.set_overlay_merge(False) is False     # the per-call switch was put back
        assert "NativeUtils" not in capfd.readouterr().err
    finally:
        native.set_overlay_merge(prev)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from livescan3d_amd import native
from tests import merge_cases
rig = merge_cases.wall(3)
v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                            generate_triangles=True)
err = native.last_error()
on = native.set_overlay_merge(True)
print("RESULT", int(on), len(t), repr(err))
"""


def test_env_switch_in_child_process(gpu, orc):
    """$LSN_OVERLAY_MERGE=1 switches the merge on for a fresh process (one child, under a time limit)."""
    line = child(CHILD, {"LSN_OVERLAY_MERGE": "1"}, ROOT)[0].split(" ", 3)
    assert line[0] == "RESULT"
    want, _ = merge_ref.overlay_merge(merge_cases.wall(3), orc)
    assert line[1] == "1" and int(line[2]) == len(want) and line[3] == "''"
