"""lsnFusionRenderViews / lsnFusionRenderDiagnostics / lsnLastMeshRenderView on the GPU against the CPU restatement (tests/render_ref.py).

Bar: bit-exact -- every depth and colour byte of every tick and view equals the restatement's, the diagnostics' drawn / pixel counts
equal its counts.  Every test fails without the feature (the exports are missing)."""
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, merge_cases, render_ref
from tests.support import ROOT, Clouds, Guarded, child, export

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_merge_ref.npz")


def _golden_clouds():
    g = np.load(GOLDEN)
    W, H = (int(v) for v in g["size"])
    intr = render_ref.intrinsics(W, H)
    rng = np.random.default_rng(1)
    out = []
    for k in range(int(g["n_draw"])):
        t9 = g[f"draw_tris_{k}"]
        out.append(render_ref.soup(t9, intr, rng.integers(0, 256, (3 * len(t9), 3))))
    return out, intr, W, H, g


def test_golden_triangle_sets(gpu):
    """The eight triangle sets of the reference's own drawTriangle fixture at 48 x 40, each a one-sensor, one-tick cloud: the image is the
    restatement's, and its depth the reference's."""
    import torch
    clouds, intr, W, H, g = _golden_clouds()
    for k, cloud in enumerate(clouds):
        c = Clouds(torch, [cloud])
        depth, _, _ = c.check(intr, render_ref.IDENTITY, W, H)
        assert np.array_equal(depth[0, 0], g[f"draw_depth_{k}"]), k
        c.check(intr, render_ref.IDENTITY, W, H, points=True)
        c.close()


@pytest.fixture(scope="module")
def ring_fusion(gpu):
    from livescan3d_amd.fusion import DeviceFusion
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    fus = DeviceFusion.from_rigs([rig])
    fus.run_mesh()
    yield rig, fus
    fus.close()


def _check_fusion(fus, intr, wt, w, h, points, tick=0):
    depth, rgb = fus.render_views(intr, wt, w, h, points=points)
    verts, _ = fus.tick_cloud(tick)
    tris = fus.tick_triangles(tick)
    depth, rgb = depth.cpu().numpy().view(np.uint16), rgb.cpu().numpy()
    wd, wc, info = render_ref.render_views(verts, None if points else tris, intr, wt, w, h)
    assert np.array_equal(depth[tick], wd), int((depth[tick] != wd).sum())
    assert np.array_equal(rgb[tick], wc)
    for q, i in enumerate(info):
        d = fus.plan.render_diagnostics(tick, q)
        assert d["drawn"] == i["drawn"] and d["pixels"] == i["pixels"], (q, d, i)
    return depth, rgb, info


@pytest.mark.parametrize("points", [False, True])
def test_ring_rig_views_and_sizes(ring_fusion, points):
    rig, fus = ring_fusion
    views = render_ref.ring_views(rig)
    for (w, h), intr in (((96, 80), rig.intr[:7]), ((64, 48), render_ref.intrinsics(64, 48, 45.0)), ((1, 1), render_ref.TINY_INTR[(1, 1)]),
                         ((1024, 3), render_ref.TINY_INTR[(1024, 3)])):
        depth, rgb, info = _check_fusion(fus, np.tile(intr, 4), views, w, h, points)
        assert not depth[0, 3].any() and not rgb[0, 3].any()                     # looking away
        assert info[1]["pixels"] > 0 or (w == 1 and not points)
        # four views in one call equal four calls of one view
        for q in range(4):
            d1, c1 = fus.render_views(intr, views[q], w, h, points=points)
            assert np.array_equal(d1.cpu().numpy().view(np.uint16)[0, 0], depth[0, q]) and np.array_equal(c1.cpu().numpy()[0, 0], rgb[0, q])


def test_after_overlay_merge_and_colour_transfer(gpu):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = merge_cases.wall(4, 96, 80)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        n_before = len(fus.tick_triangles(0))
        fus.overlay_merge()
        fus.color_transfer()
        torch.cuda.synchronize()
        assert len(fus.tick_triangles(0)) < n_before      # the merge dropped what the views share
        views = render_ref.ring_views(rig)[:2]
        _, _, info = _check_fusion(fus, np.tile(rig.intr[:7], 2), views, 96, 80, False)
        assert info[0]["pixels"] > 500


def _squares(sides, w=64, h=48):
    """Two triangles per square of side s, at distinct depths, overlapping.  Rows of drawTriangle's {x, y, d} x 3."""
    rows = []
    for s in sides:
        x0, y0, d = (7 * s) % (w - s), (5 * s) % (h - s), 3000 - 40 * s
        rows += [[x0, y0, d, x0, y0 + s, d + 3, x0 + s, y0, d + 5], [x0 + s, y0, d + 5, x0, y0 + s, d + 3, x0 + s, y0 + s, d + 8]]
    return rows


def test_work_list_path(gpu):
    """Squares of side 1 .. 40 px: whatever the box size above which a triangle is drawn by a whole wave, the sweep crosses it."""
    import torch
    intr = render_ref.intrinsics(64, 48)
    rng = np.random.default_rng(2)
    colours = lambda rows: rng.integers(0, 256, (3 * len(rows), 3))
    sets = [_squares([1]), _squares([40]), _squares(range(1, 41))]
    c = Clouds(torch, [render_ref.soup(r, intr, colours(r)) for r in sets])
    depth, _, diags = c.check(intr, render_ref.IDENTITY, 64, 48)
    assert diags[0]["large"] == 0 and diags[0]["pixels"] >= 1
    assert diags[1]["large"] == 2 and diags[1]["pixels"] >= 40 * 40
    assert 0 < diags[2]["large"] < 80 and diags[2]["drawn"] == 80
    c.close()
    # two view-filling coincident triangles: the lower index
    one = [0, 0, 1500, 0, 47, 1700, 63, 0, 1900]
    c = Clouds(torch, [render_ref.soup([one, one], intr, [[250, 10, 10]] * 3 + [[10, 10, 250]] * 3)])
    depth, rgb, diags = c.check(intr, render_ref.IDENTITY, 64, 48)
    assert diags[0]["large"] == 2 and (depth[0, 0] != 0).sum() > 1400
    assert set(map(tuple, rgb[0, 0][depth[0, 0] != 0])) == {(250, 10, 10)}
    c.close()


def test_batch_and_buffer_hygiene(gpu):
    """Three ticks with a mesh each, one of them empty, one with indices out of range; then a smaller and a larger view on the same plan:
    the keys were left at "none" and the scratch grows."""
    import torch
    clouds, intr, W, H, _ = _golden_clouds()
    v7, t7 = clouds[7]
    bad = np.concatenate([t7[:200], [[0, 1, len(v7)], [-1, 2, 3], [2 ** 30, 0, 1]], t7[200:]]).astype(np.int32)
    c = Clouds(torch, [clouds[0], (v7[:0], t7[:0]), (v7, bad)])
    c.check(intr, render_ref.IDENTITY, W, H)
    c.check(render_ref.intrinsics(16, 12, 16.0), render_ref.IDENTITY, 16, 12)
    two = np.stack([render_ref.IDENTITY, render_ref.pose_at(np.eye(3), [0.05, -0.02, -0.1])])
    c.check(np.tile(render_ref.intrinsics(200, 150, 190.0), 2), two, 200, 150)
    c.check(intr, render_ref.IDENTITY, W, H, points=True)
    c.check(intr, render_ref.IDENTITY, W, H)
    c.close()


def test_bad_arguments_touch_nothing(gpu):
    import torch
    clouds, intr, W, H, _ = _golden_clouds()
    c = Clouds(torch, [clouds[1]])
    with pytest.raises(native.NativeUtilsError, match="nothing has been rendered"):
        c.plan.render_diagnostics(0, 0)
    gd, gc = Guarded(torch, 17 * W * H * 2, "cuda"), Guarded(torch, 17 * W * H * 3, "cuda")
    call = lambda i, t, w, h, v=c.v.data_ptr(): c.plan.render_views(i, t, w, h, v, c.off.data_ptr(), c.t.data_ptr(), c.toff.data_ptr(), gd.ptr, gc.ptr)
    for args, msg in (((np.tile(intr, 17), np.tile(render_ref.IDENTITY, 17), W, H), "views"), ((np.zeros(0), np.zeros(0), W, H), "views"),
                      ((intr, render_ref.IDENTITY, 0, H), "pixels"), ((intr, render_ref.IDENTITY, W, 1025), "pixels"),
                      ((intr, render_ref.IDENTITY, -1, -1), "pixels"), ((intr, render_ref.IDENTITY, W, H, 0), "null")):
        with pytest.raises(native.NativeUtilsError, match=msg):
            call(*args)
    torch.cuda.synchronize()
    assert bool((gd.buf == 0xA5).all().item()) and bool((gc.buf == 0xA5).all().item())
    c.check(intr, render_ref.IDENTITY, W, H)     # and the plan still renders
    with pytest.raises(native.NativeUtilsError, match="last render"):
        c.plan.render_diagnostics(0, 1)
    c.close()


def _check_last_mesh(rig, v, t):
    view = render_ref.ring_views(rig)[1]
    w, h = int(rig.widths[0]), int(rig.heights[0])
    for points in (False, True):
        depth, rgb, n = native.last_mesh_render_view(rig.intr[:7], view, w, h, points_only=points)
        wd, wc, info = render_ref.render(v, None if points else t, rig.intr[:7], view, w, h)
        assert np.array_equal(depth, wd) and np.array_equal(rgb, wc) and n == info["pixels"] > 0


def test_last_mesh_export(gpu):
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    v, t, err = export(rig)
    assert err == "" and len(t) > 0
    _check_last_mesh(rig, v, t)
    wall = merge_cases.wall(4, 96, 80)
    v2, t2, err = export(wall, generate_triangles=True, overlay_merge=True)
    assert err == "" and len(t2) > 0
    _check_last_mesh(wall, v2, t2)
    with pytest.raises(native.NativeUtilsError, match="pixels"):
        native.last_mesh_render_view(rig.intr[:7], rig.wt[:12], 0, 5)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from livescan3d_amd import native
from tests import color_cases, render_ref
rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
view = render_ref.ring_views(rig)[1]
try:
    native.last_mesh_render_view(rig.intr[:7], view, 96, 80)
    first = "rendered"
except native.NativeUtilsError as ex:
    first = str(ex)
v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
shards = native.host_shards(3, 0)[1]
depth, rgb, n = native.last_mesh_render_view(rig.intr[:7], view, 96, 80)
wd, wc, info = render_ref.render(v, t, rig.intr[:7], view, 96, 80)
print("RESULT", int(np.array_equal(depth, wd) and np.array_equal(rgb, wc) and n == info["pixels"] > 0), len(shards.split()), repr(first))
"""


def test_last_mesh_after_a_sharded_call_and_without_a_mesh(gpu):
    """A fresh process: no mesh yet -> -1 and a message; then a merge call sharded over two lanes of the one GPU ($LSN_HOST_DEVICES=0,0),
    whose mesh exists in host memory only and is rebuilt for the render."""
    line = child(CHILD, {"LSN_HOST_DEVICES": "0,0"}, ROOT)[0].split(" ", 3)
    assert line[0] == "RESULT" and line[1] == "1" and line[2] == "2", line
    assert "no mesh is resident" in line[3], line
