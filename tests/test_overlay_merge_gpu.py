"""generateMeshFromDepthMaps(bgenerate_triangles = true) with the overlay merge switched on, and lsnFusionOverlayMerge, on the GPU
against the CPU reference (tests/merge_ref.py).

Bar: bit-exact -- the triangles equal the reference's; the vertices are byte-identical to the call without the merge; the
diagnostics (reprojected maps, final maps, point_assigned) equal the reference's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, color_ref, merge_cases, merge_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT_BOUNDS = np.array([-0.3, -1.0, -1.5, 1.5, 1.5, 1.5], dtype=np.float32)   # through the sphere, inside the views' overlap


def _export(rig, color=False, tri=True, merge=True):
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                color_transfer=color, generate_triangles=tri, overlay_merge=merge)
    return v, t, native.last_error()


def _device(rigs, order=("merge",)):
    """run_mesh over a batch of ticks, then the stages of `order` ("merge", "color").  Returns (plan, verts, off, tris per tick)."""
    import torch
    T = len(rigs)
    plan = native.FusionPlan(0, T, rigs[0].widths, rigs[0].heights)
    plan.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
    depth = torch.from_numpy(np.stack([r.depth_maps.view(np.int16) for r in rigs])).cuda()
    rgb = torch.from_numpy(np.stack([r.depth_colors for r in rigs])).cuda()
    N, cap = rigs[0].n, plan.capacity
    verts = torch.zeros((T, cap, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((T, N + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((T, 2 * cap, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((T, N + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)
    plan.run_mesh(depth.data_ptr(), rgb.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
    for stage in order:
        if stage == "merge":
            plan.overlay_merge(depth.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
        else:
            plan.color_transfer(depth.data_ptr(), verts.data_ptr(), off.data_ptr(), st)
    torch.cuda.synchronize()
    o, to, tr = off.cpu().numpy(), toff.cpu().numpy(), tri.cpu().numpy()
    return plan, verts.cpu().numpy(), o, [tr[k, :int(to[k, -1])] for k in range(T)]


def _check_device(rig, orc, expect_assigned=None):
    plan, verts, off, tris = _device([rig])
    want, diag = merge_ref.overlay_merge(rig, orc)
    assert tris[0].shape == want.shape and np.array_equal(tris[0], want), (tris[0].shape, want.shape)
    nv = int(off[0, -1])
    d = plan.overlay_diagnostics(0, nv)
    assert np.array_equal(d["reprojected"], diag["reprojected"])
    assert np.array_equal(d["merged"], diag["merged"])
    assert np.array_equal(d["assigned"], diag["assigned"]) and d["n_assigned"] == int(diag["assigned"].sum())
    if expect_assigned is not None:
        assert (d["n_assigned"] > 0) == expect_assigned, d["n_assigned"]
    return want, diag


def _check_export(rig, orc):
    plain, t0, e0 = _export(rig, merge=False, tri=False)
    got, t1, e1 = _export(rig)
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
    _, plain_tris, _ = _export(rig, merge=False, tri=False)
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
    _, plain, _ = _export(rig, merge=False, tri=False)
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
    _, _, _, tris = _device(rigs)
    for k in range(T):
        _, _, _, one = _device([rigs[k]])
        assert np.array_equal(tris[k], one[0]), k
    want, _ = merge_ref.overlay_merge(rigs[5], orc)
    assert np.array_equal(tris[5], want)


def test_merge_and_colour_in_both_orders(gpu, orc):
    rig = merge_cases.wall(4)
    _, v1, _, t1 = _device([rig], ("merge", "color"))
    _, v2, _, t2 = _device([rig], ("color", "merge"))
    want, _ = merge_ref.overlay_merge(rig, orc)
    cwant, _ = color_ref.color_transfer(rig, orc)
    assert np.array_equal(t1[0], want) and np.array_equal(t2[0], want)
    assert v1.tobytes() == v2.tobytes() and v1[0, :len(cwant)].tobytes() == cwant.tobytes()
    got, tris, err = _export(rig, color=True)
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
    plain, t0, _ = _export(rig, merge=False)
    got, t1, err = _export(rig)
    assert "same size" in err and got.tobytes() == plain.tobytes() and np.array_equal(t0, t1)


def test_switch_off_behaves_as_before(gpu):
    rig = color_cases.ring(4, sizes=[(256, 212)] * 4, of=8)
    prev = native.set_overlay_merge(False)
    try:
        v0, t0, e0 = _export(rig, merge=None)
        assert "overlay merge are outside this library's scope" in e0
        plain, tp, _ = _export(rig, merge=None, tri=False)
        assert v0.tobytes() == plain.tobytes() and np.array_equal(t0, tp)
    finally:
        native.set_overlay_merge(prev)


def test_switch_is_restored_and_silent(gpu, capfd):
    prev = native.set_overlay_merge(False)
    try:
        _export(merge_cases.wall(2), merge=True)
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
    env = dict(os.environ, LSN_OVERLAY_MERGE="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT")][-1].split(" ", 3)
    want, _ = merge_ref.overlay_merge(merge_cases.wall(3), orc)
    assert line[1] == "1" and int(line[2]) == len(want) and line[3] == "''"
