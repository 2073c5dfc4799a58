"""lsnFusionSimplify / lsnFusionSimplifyDiagnostics / lsnLastMeshTransferFrameLod / lsnLastMeshPlyLod on the GPU against the CPU restatement
(tests/simplify_ref.py).

Bar: bit-exact -- vertices, both offset rows, triangles, remap and the diagnostics' three counts of every tick equal the restatement's;
every output lies between guard bands in a buffer prefilled with 249, and nothing behind a tick's new counts is written
(tests/simplify_cases.py check_device).  Every test fails without the feature (the exports are missing)."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, merge_cases, render_ref, simplify_ref
from tests.simplify_cases import PREFILL, Clouds, Outputs, cases, check_device
from tests.support import ROOT, child, export
from tests.test_simplify_ref import RING_KEPT

pytestmark = pytest.mark.gpu

CELLS = (0.1, 0.25, 0.5)     # the cells of the hand-made cases


def _tick(name):
    xyz, off, tri, toff, _ = cases()[name]
    return simplify_ref.cloud(xyz), off, tri, toff


def test_hand_made_clouds(gpu):
    """One 8 x 8 sensor, a case per tick; every cell of the cases on every tick."""
    import torch
    c = Clouds(torch, [_tick(k) for k in ("two_in_one_cell", "negative_coordinates", "on_the_boundary", "unclustered", "triangles")])
    for cell in CELLS:
        _, refs = c.check(cell)
        c.check(cell, points=True, with_remap=False)
    assert refs[3]["unclustered"] == 9 and refs[3]["cells"] == 12          # cell 0.5, the "unclustered" case
    _, refs = c.check(0.1)
    assert refs[4]["triangles"].tolist() == [[1, 2, 3], [0, 1, 2], [0, 1, 2], [3, 2, 1], [2, 3, 0]] and refs[4]["dropped_triangles"] == 6
    c.close()
    c = Clouds(torch, [_tick("two_sensors")], sizes=((4, 4),) * 4)
    _, refs = c.check(0.1)
    assert refs[0]["offsets"].tolist() == [0, 3, 3, 4, 4] and refs[0]["tri_offsets"].tolist() == [0, 1, 1, 3, 4]
    c.close()


def test_full_table_probe_chains(gpu):
    """64 vertices per tick, the 8 x 8 sensor's capacity, so the tick's table has 128 slots at load 0.5: 64 distinct cells (random ones in
    eight ticks, a row of neighbours, a diagonal), 64 vertices in one cell, 32 cells of two.  Probe chains and the wrap-around at the
    table's end show as a wrong representative."""
    import torch
    rng = np.random.default_rng(11)
    ticks = []
    for _ in range(8):
        q = rng.choice(2 ** 15, 64, replace=False)
        ticks.append(np.stack([q % 32, (q // 32) % 32, q // 1024], axis=1) - 16.0)
    line = np.arange(64.0)
    ticks += [np.stack([line, 0 * line, 0 * line], axis=1), np.stack([line, line, line], axis=1) - 32.0, np.zeros((64, 3)) + 0.5,
              np.stack([line // 2, 0 * line, -(line // 2)], axis=1)]
    fan = np.stack([np.arange(62), np.arange(62) + 1, np.arange(62) + 2], axis=1).astype(np.int32)
    c = Clouds(torch, [(simplify_ref.cloud(x * 0.1 + 0.05), [0, 64], fan, [0, 62]) for x in ticks])
    _, refs = c.check(0.1)
    assert [r["cells"] for r in refs] == [64] * 10 + [1, 32]
    assert all(np.array_equal(r["triangles"], fan) for r in refs[:10]) and len(refs[10]["triangles"]) == 0
    c.check(np.inf)          # inv = 0: one cell
    c.check(1e-40)           # inv = inf: all unclustered
    c.close()


def test_more_tiles_than_one_scan_round(gpu):
    """The kept vertices and triangles are counted per tile of 256 and one workgroup turns a tick's counts into prefixes, 1024 a round
    with the sum carried along.  1026 vertex tiles and as many triangle tiles, nearly every vertex alone in its cell: the second round's
    tiles have something to add to and the kept vertices themselves fill more than 1024 tiles.  One sensor of 513 x 513, the smallest
    square capacity above 1024 tiles."""
    import torch
    nv = 263000                                               # of the 263169 the sensor holds: 1028 tiles
    rng = np.random.default_rng(3)
    fan = (np.arange(nv - 2, dtype=np.int32)[:, None] + np.arange(3, dtype=np.int32)[None, :])
    c = Clouds(torch, [(simplify_ref.cloud(rng.uniform(-2.0, 2.0, (nv, 3))), [0, nv], fan, [0, nv - 2])], sizes=((513, 513),))
    _, refs = c.check(0.01)                                   # 400^3 cells: some 540 vertices share one (nv^2 / 2 / 400^3)
    assert refs[0]["cells"] > 1024 * 256 and len(refs[0]["triangles"]) > nv - 2 - 3 * 2000
    c.close()


@pytest.fixture(scope="module")
def ring_fusion(gpu):
    from livescan3d_amd.fusion import DeviceFusion
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    fus = DeviceFusion.from_rigs([rig])
    fus.run_mesh()
    yield rig, fus
    fus.close()


def _check_fusion(fus, cell, points=False, with_remap=True):
    import torch
    return check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, cell, points, with_remap)


@pytest.mark.parametrize("cell", sorted(RING_KEPT))
def test_ring_known_answers_and_idempotence(ring_fusion, cell):
    import torch
    _, fus = ring_fusion
    out, refs = _check_fusion(fus, cell)
    assert refs[0]["cells"] == RING_KEPT[cell]
    if cell == 0.05:
        assert refs[0]["offsets"].tolist() == [0, 1958, 3500, 5040]
    # the output once more: the same bytes
    T, n, cap = 1, fus.n_maps, fus.capacity
    first = out.host()
    body = lambda k, dt, shape: out.g[k].body().view(dt).reshape(shape)
    v1, off1 = body("v", torch.uint8, (T, cap, 16)), body("off", torch.int32, (T, n + 1))
    t1, toff1 = body("t", torch.int32, (T, 2 * cap, 3)), body("toff", torch.int32, (T, n + 1))
    out2, refs2 = check_device(torch, fus.plan, v1, off1, t1, toff1, cell)
    second = out2.host()
    for k in ("v", "off", "t", "toff"):
        assert np.array_equal(first[k], second[k]), k
    assert refs2[0]["remap"].tolist() == list(range(refs[0]["cells"]))


def test_ring_points_mode_and_the_thin_method(ring_fusion):
    import torch
    from livescan3d_amd.fusion import SENTINEL
    _, fus = ring_fusion
    _, refs = _check_fusion(fus, 0.05, points=True)
    _check_fusion(fus, 0.05, with_remap=False)
    v, off, t, toff, remap = fus.simplify(0.05)
    torch.cuda.synchronize()
    nv, nt = int(off[0, -1]), int(toff[0, -1])
    assert nv == 5040 and np.array_equal(v[0, :nv].cpu().numpy(), refs[0]["vertices"].view(np.uint8).reshape(-1, 16))
    assert np.array_equal(remap[0, :len(refs[0]["remap"])].cpu().numpy(), refs[0]["remap"]) and nt > 0
    v, off, t, toff, remap = fus.simplify(0.05, points=True)
    torch.cuda.synchronize()
    assert t is None and toff is None and off[0].tolist() == [0, 1958, 3500, 5040] and SENTINEL == -7


def test_after_overlay_merge(gpu):
    """The merge rewrites the triangles: they are no grid triangles any more."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = merge_cases.wall(4, 96, 80)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        n_before = len(fus.tick_triangles(0))
        fus.overlay_merge()
        torch.cuda.synchronize()
        assert 0 < len(fus.tick_triangles(0)) < n_before
        for cell in (0.02, 0.05):
            _, refs = _check_fusion(fus, cell)
            assert 0 < len(refs[0]["triangles"]) and refs[0]["cells"] < len(refs[0]["remap"])


def test_three_ticks_of_different_frames(gpu):
    """Tick 1 has no valid depth (0 vertices); then the whole plan with an empty crop box."""
    import copy
    from livescan3d_amd.fusion import DeviceFusion
    rigs = [color_cases.ring(3, sizes=[(96, 80)] * 3, tick=k) for k in range(3)]
    rigs[1] = copy.copy(rigs[1])
    rigs[1].depth_maps = np.zeros_like(rigs[1].depth_maps)
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run_mesh()
        _, refs = _check_fusion(fus, 0.05)
        counts = [len(r["remap"]) for r in refs]
        assert counts[0] > 10000 and counts[1] == 0 and counts[2] > 10000 and refs[0]["cells"] != refs[2]["cells"]
        _check_fusion(fus, 0.05, points=True)
        fus.set_params(rigs[0].intr, rigs[0].wt, np.array([1, 1, 1, -1, -1, -1], np.float32))
        fus.run_mesh()
        _, refs = _check_fusion(fus, 0.05)
        assert [len(r["remap"]) for r in refs] == [0, 0, 0]


def test_mixed_sizes(gpu):
    from livescan3d_amd.fusion import DeviceFusion
    rig = color_cases.ring(3, sizes=[(37, 17), (1, 1), (17, 37)])
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        for cell in (0.05, 0.2):
            _, refs = _check_fusion(fus, cell)
            off = fus.host_offsets()[0]
            assert off[2] - off[1] <= 1 and refs[0]["cells"] < off[3]
            _check_fusion(fus, cell, points=True)


def test_switch_off_and_errors(ring_fusion):
    import torch
    _, fus = ring_fusion
    plan, cap, n = fus.plan, fus.capacity, fus.n_maps
    nv, nt = int(fus.host_offsets()[0, -1]), int(fus.host_tri_offsets()[0, -1])
    # triangles that a cell > 0 would drop are copied as they are
    tri = fus.triangles.clone()
    tri[0, 5] = torch.tensor([0, 0, 0], dtype=torch.int32)
    tri[0, 6] = torch.tensor([-1, 2, cap + 5], dtype=torch.int32)
    for cell in (0.0, -1.0, float("nan")):
        _, refs = check_device(torch, plan, fus.vertices, fus.offsets, tri, fus.tri_offsets, cell)
        assert len(refs[0]["vertices"]) == nv and len(refs[0]["triangles"]) == nt and refs[0]["triangles"][6].tolist() == [-1, 2, cap + 5]
    _, refs = check_device(torch, plan, fus.vertices, fus.offsets, tri, fus.tri_offsets, 0.05)
    assert refs[0]["dropped_triangles"] > 2

    def refused(out, msg, **ptrs):
        a = {"v": fus.vertices.data_ptr(), "off": fus.offsets.data_ptr(), "t": fus.triangles.data_ptr(), "toff": fus.tri_offsets.data_ptr(),
             "v_out": out.ptr("v"), "off_out": out.ptr("off"), "t_out": out.ptr("t"), "toff_out": out.ptr("toff"), "remap": out.ptr("remap")}
        a.update(ptrs)
        with pytest.raises(native.NativeUtilsError, match=msg):
            plan.simplify(0.05, a["v"], a["off"], a["t"], a["toff"], a["v_out"], a["off_out"], a["t_out"], a["toff_out"], a["remap"])

    out = Outputs(torch, 1, n, cap)
    before = {k: t.clone() for k, t in (("v", fus.vertices), ("off", fus.offsets), ("t", fus.triangles), ("toff", fus.tri_offsets))}
    refused(out, "overlaps", v_out=fus.vertices.data_ptr())                              # in place
    refused(out, "overlaps", v_out=fus.vertices.data_ptr() + 16 * (cap - 1))            # the last input vertex under the first output one
    refused(out, "overlaps", v=out.ptr("v") + 16 * (cap - 1))
    refused(out, "overlaps", remap=fus.triangles.data_ptr() + 12 * 2 * cap - 4)
    refused(out, "overlaps", toff_out=fus.offsets.data_ptr())
    refused(out, "null", v_out=0)
    refused(out, "null", off=0)
    refused(out, "null", toff_out=0)
    torch.cuda.synchronize()
    assert out.untouched()
    for k, t in (("v", fus.vertices), ("off", fus.offsets), ("t", fus.triangles), ("toff", fus.tri_offsets)):
        assert torch.equal(before[k], t), k
    L = native.lib()
    assert L.lsnFusionSimplify(None, 0.05, fus.vertices.data_ptr(), fus.offsets.data_ptr(), None, None, out.ptr("v"), out.ptr("off"), None, None,
                               None, None) == -1 and "null" in native.last_error()
    assert L.lsnFusionSimplifyDiagnostics(None, 0, None, None, None, None) == -1
    torch.cuda.synchronize()
    assert out.untouched()
    fresh = native.FusionPlan(0, 1, [8], [8])
    with pytest.raises(native.NativeUtilsError, match="nothing has been simplified"):
        fresh.simplify_diagnostics(0)
    fresh.close()
    with pytest.raises(native.NativeUtilsError, match="last call had 1 ticks"):
        plan.simplify_diagnostics(1)
    _check_fusion(fus, 0.05)          # and the plan still simplifies


def test_downstream_pack_ply_and_render(ring_fusion, orc):
    """The simplified tick goes into lsnTransferPack, lsnPlyPack and lsnFusionRenderViews as it is."""
    import torch
    rig, fus = ring_fusion
    cap = fus.capacity
    out, refs = _check_fusion(fus, 0.05)
    r = refs[0]
    nv, nt = len(r["vertices"]), len(r["triangles"])
    bound = native.transfer_frame_bound(nv, nt)
    wire = torch.zeros(bound + 64, dtype=torch.uint8, device="cuda")
    packer = native.TransferPacker(0, nv, nt)
    n = packer.pack(out.ptr("v"), nv, out.ptr("t"), nt, wire.data_ptr(), bound)
    assert wire[:n].cpu().numpy().tobytes() == orc.transfer_frame(r["vertices"], r["triangles"]) and packer.last_path() == 2
    packer.close()
    need = native.ply_binary_bytes(nv, nt)
    ply = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")
    assert native.ply_pack(0, out.ptr("v"), nv, out.ptr("t"), nt, ply.data_ptr(), need) == need
    torch.cuda.synchronize()
    assert ply[:need].cpu().numpy().tobytes() == orc.ply_binary(r["vertices"], r["triangles"])
    views = render_ref.ring_views(rig)[:2]
    intr = np.tile(rig.intr[:7], 2)
    for points in (False, True):
        depth = torch.zeros((1, 2, 80, 96), dtype=torch.int16, device="cuda")
        rgb = torch.zeros((1, 2, 80, 96, 3), dtype=torch.uint8, device="cuda")
        fus.plan.render_views(intr, views, 96, 80, out.ptr("v"), out.ptr("off"), 0 if points else out.ptr("t"), 0 if points else out.ptr("toff"),
                              depth.data_ptr(), rgb.data_ptr())
        torch.cuda.synchronize()
        wd, wc, info = render_ref.render_views(r["vertices"], None if points else r["triangles"], intr, views, 96, 80)
        assert np.array_equal(depth.cpu().numpy().view(np.uint16)[0], wd) and np.array_equal(rgb.cpu().numpy()[0], wc)
        assert info[1]["pixels"] > 500


def _restated(v, t, cell):
    r = simplify_ref.simplify(v, [0, len(v)], t if len(t) else None, [0, len(t)], cell)
    return r["vertices"], (r["triangles"] if len(t) else np.zeros((0, 3), np.int32))


def test_host_exports(gpu, orc):
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    v, t, err = export(rig)
    assert err == "" and len(v) == 11087 and len(t) > 0
    plain = native.last_mesh_transfer_frame(), native.last_mesh_ply()
    assert plain == (orc.transfer_frame(v, t), orc.ply_binary(v, t))
    for cell in (0.05, 0.2, 100.0):
        rv, rt = _restated(v, t, cell)
        frame, ply = native.last_mesh_transfer_frame_lod(cell), native.last_mesh_ply_lod(cell)
        assert frame == orc.transfer_frame(rv, rt), cell
        assert ply == orc.ply_binary(rv, rt), cell
        assert len(frame) < len(plain[0]) and len(ply) < len(plain[1])
    assert len(_restated(v, t, 0.05)[0]) == 5040
    for cell in (0.0, -1.0, float("nan")):
        assert (native.last_mesh_transfer_frame_lod(cell), native.last_mesh_ply_lod(cell)) == plain
    L = native.lib()
    assert L.lsnLastMeshTransferFrameLod(0.05, None, 0) >= len(plain[0]) and L.lsnLastMeshPlyLod(0.05, None, 0) >= len(plain[1])
    small = np.zeros(100, np.uint8)
    assert L.lsnLastMeshPlyLod(0.05, small.ctypes.data, 100) == -1 and "buffer holds" in native.last_error()
    # the resident mesh is as it was
    assert (native.last_mesh_transfer_frame(), native.last_mesh_ply()) == plain
    # a cloud without triangles
    rig1 = color_cases.ring(1, sizes=[(64, 48)], of=3)
    v1 = native.generate_vertices_from_depth_map(rig1.depth_maps, rig1.depth_colors, rig1.widths, rig1.heights, rig1.intr, rig1.wt, rig1.bounds, 0)
    none = np.zeros((0, 3), np.int32)
    rv, _ = _restated(v1, none, 0.1)
    assert 0 < len(rv) < len(v1)
    assert native.last_mesh_transfer_frame_lod(0.1) == orc.transfer_frame(rv, none) and native.last_mesh_ply_lod(0.1) == orc.ply_binary(rv, none)


CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from livescan3d_amd import native
from oracle import orc
from tests import color_cases, simplify_ref
orc.build()
rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
try:
    native.last_mesh_ply_lod(0.05)
    first = "packed"
except native.NativeUtilsError as ex:
    first = str(ex)
v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
shards = native.host_shards(3, 0)[1]
r = simplify_ref.simplify(v, [0, len(v)], t, [0, len(t)], 0.05)
ok = native.last_mesh_transfer_frame_lod(0.05) == orc.transfer_frame(r["vertices"], r["triangles"]) and \
    native.last_mesh_ply_lod(0.05) == orc.ply_binary(r["vertices"], r["triangles"])
print("RESULT", int(ok), len(shards.split()), repr(first))
"""


def test_host_exports_after_a_sharded_call_and_without_a_mesh(gpu, orc):
    """A fresh process: no mesh yet -> -1 and a message; then a merge call sharded over two lanes of the one GPU ($LSN_HOST_DEVICES=0,0),
    whose mesh exists in host memory only and is rebuilt for the stage."""
    line = child(CHILD, {"LSN_HOST_DEVICES": "0,0"}, ROOT)[0].split(" ", 3)
    assert line[0] == "RESULT" and line[1] == "1" and line[2] == "2", line
    assert "no mesh is resident" in line[3], line


def test_plans_release_their_scratch(gpu):
    """Two plans created, simplified and destroyed, again and again, must not lose HBM (as test_handles_release_their_device_memory of
    tests/test_wire_gpu.py checks the other handles)."""
    import torch
    rig = color_cases.ring(2, sizes=[(512, 424)] * 2, of=8)

    def cycle():
        from livescan3d_amd.fusion import DeviceFusion
        pair = [DeviceFusion.from_rigs([rig]) for _ in range(2)]
        for fus in pair:
            fus.run_mesh()
            fus.simplify(0.02)
            fus.simplify(0.0, points=True)
        torch.cuda.synchronize()
        assert pair[0].plan.simplify_diagnostics(0)["cells"] > 1000
        for fus in pair:
            fus.close()

    cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(6):
        cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 16 << 20, f"{(free0 - free1) >> 20} MiB of HBM lost over 6 create/simplify/destroy cycles"
