"""lsnFusionFragments / lsnFusionFragmentsDiagnostics / lsnLastMeshTransferFrameFragments / lsnLastMeshPlyFragments on the GPU against the
CPU restatement (tests/fragments_ref.py).

Bar: bit-exact -- vertices, both offset rows, triangles, remap, labels and the diagnostics' four counts of every tick equal the
restatement's; every output lies between guard bands in a buffer prefilled with 249, and nothing behind a tick's new counts is written
(tests/fragments_cases.py check_device).  Every test fails without the feature (the exports are missing)."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, fragments_ref, normals_cases, normals_ref, simplify_cases, simplify_ref
from tests.fragments_cases import Outputs, cases, check_device, clouds
from tests.support import export

pytestmark = pytest.mark.gpu

CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_case(gpu, name):
    """The case's ticks as one batch, every min_vertices of the case; the first one again without the nullable outputs, one at a time."""
    import torch
    case = CASES[name]
    c = clouds(torch, case)
    try:
        for m in case.mins:
            check_device(torch, c.plan, c.v, c.off, c.t, c.toff, m)
        check_device(torch, c.plan, c.v, c.off, c.t, c.toff, case.mins[0], with_remap=False, with_labels=False)
        check_device(torch, c.plan, c.v, c.off, c.t, c.toff, case.mins[0], with_remap=False)
        check_device(torch, c.plan, c.v, c.off, c.t, c.toff, case.mins[0], with_labels=False)
    finally:
        c.close()


@pytest.fixture(scope="module")
def ring_fusion(gpu):
    from livescan3d_amd.fusion import DeviceFusion
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    fus = DeviceFusion.from_rigs([rig])
    fus.run_mesh()
    yield rig, fus
    fus.close()


def _check_fusion(fus, m, **kw):
    import torch
    return check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, m, **kw)


def test_diagnostics_before_any_call_and_out_of_range(ring_fusion):
    fresh = native.FusionPlan(0, 1, [8], [8])
    with pytest.raises(native.NativeUtilsError, match="nothing has been filtered"):
        fresh.fragments_diagnostics(0)
    fresh.close()
    _, fus = ring_fusion
    _check_fusion(fus, 64)
    for tick in (1, -1):
        with pytest.raises(native.NativeUtilsError, match="last call had 1 ticks"):
            fus.plan.fragments_diagnostics(tick)
    assert native.lib().lsnFusionFragmentsDiagnostics(None, 0, None, None, None, None, None) == -1


def test_arguments_are_refused_with_nothing_touched(ring_fusion):
    import torch
    _, fus = ring_fusion
    plan, cap, n = fus.plan, fus.capacity, fus.n_maps

    def refused(out, msg, **ptrs):
        a = {"v": fus.vertices.data_ptr(), "off": fus.offsets.data_ptr(), "t": fus.triangles.data_ptr(), "toff": fus.tri_offsets.data_ptr(),
             "v_out": out.ptr("v"), "off_out": out.ptr("off"), "t_out": out.ptr("t"), "toff_out": out.ptr("toff"), "remap": out.ptr("remap"),
             "labels": out.ptr("labels")}
        a.update(ptrs)
        with pytest.raises(native.NativeUtilsError, match=msg):
            plan.fragments(64, a["v"], a["off"], a["t"], a["toff"], a["v_out"], a["off_out"], a["t_out"], a["toff_out"], a["remap"], a["labels"])

    out = Outputs(torch, 1, n, cap)
    before = {k: t.clone() for k, t in (("v", fus.vertices), ("off", fus.offsets), ("t", fus.triangles), ("toff", fus.tri_offsets))}
    refused(out, "overlaps", v_out=fus.vertices.data_ptr())                              # in place
    refused(out, "overlaps", v_out=fus.vertices.data_ptr() + 16 * (cap - 1))            # the last input vertex under the first output one
    refused(out, "overlaps", v=out.ptr("v") + 16 * (cap - 1))
    refused(out, "overlaps", remap=fus.triangles.data_ptr() + 12 * 2 * cap - 4)
    refused(out, "overlaps", labels=fus.vertices.data_ptr() + 16)
    refused(out, "overlaps", toff_out=fus.offsets.data_ptr())
    refused(out, "d_triangles is null", t=0)
    refused(out, "d_triangles is null", t=0, toff=0)
    for name in ("v", "off", "toff", "v_out", "off_out", "t_out", "toff_out"):
        refused(out, "null argument", **{name: 0})
    torch.cuda.synchronize()
    assert out.untouched()
    for k, t in (("v", fus.vertices), ("off", fus.offsets), ("t", fus.triangles), ("toff", fus.tri_offsets)):
        assert torch.equal(before[k], t), k
    assert native.lib().lsnFusionFragments(None, 64, fus.vertices.data_ptr(), fus.offsets.data_ptr(), fus.triangles.data_ptr(),
                                           fus.tri_offsets.data_ptr(), out.ptr("v"), out.ptr("off"), out.ptr("t"), out.ptr("toff"), None, None,
                                           None) == -1 and "null" in native.last_error()
    torch.cuda.synchronize()
    assert out.untouched()
    _check_fusion(fus, 64)            # and the plan still filters


@pytest.mark.parametrize("m", [2, 64, 256])
def test_ring_known_answers_idempotence_and_the_same_call_twice(ring_fusion, m):
    import torch
    _, fus = ring_fusion
    out, refs = _check_fusion(fus, m)
    assert refs[0]["components"] == 1471 and len(refs[0]["remap"]) == 11087
    if m == 256:
        assert (refs[0]["removed_vertices"], refs[0]["removed_components"]) == (1995, 1467)
    if m == 2:
        assert refs[0]["removed_vertices"] == 1458
    first = out.host()
    again, _ = _check_fusion(fus, m)                                     # the same call twice: the same bytes
    second = again.host()
    for k in first:
        assert np.array_equal(first[k], second[k]), k
    # the output once more: the same bytes
    out2, refs2 = check_device(torch, fus.plan, *out.tensors(torch), m)
    third = out2.host()
    for k in ("v", "off", "t", "toff"):
        assert np.array_equal(first[k], third[k]), k
    assert refs2[0]["remap"].tolist() == list(range(len(refs[0]["vertices"]))) and refs2[0]["removed_vertices"] == 0


def test_the_thin_method(ring_fusion):
    import torch
    from livescan3d_amd.fusion import SENTINEL
    _, fus = ring_fusion
    r = fragments_ref.fragments(fus.tick_cloud(0)[0], fus.host_offsets()[0], fus.tick_triangles(0), fus.host_tri_offsets()[0], 256)
    v, off, t, toff, remap, labels = fus.fragments(256)
    torch.cuda.synchronize()
    nv, nt = int(off[0, -1]), int(toff[0, -1])
    assert nv == 11087 - 1995 and np.array_equal(v[0, :nv].cpu().numpy(), r["vertices"].view(np.uint8).reshape(-1, 16))
    assert np.array_equal(t[0, :nt].cpu().numpy(), r["triangles"]) and np.array_equal(off[0].cpu().numpy(), r["offsets"])
    assert np.array_equal(remap[0, :11087].cpu().numpy(), r["remap"]) and np.array_equal(labels[0, :11087].cpu().numpy(), r["labels"])
    assert SENTINEL == -7


def _simplified(torch, out, T, n, cap):
    body = lambda k, dt, shape: out.g[k].body().view(dt).reshape(shape)
    return (body("v", torch.uint8, (T, cap, 16)), body("off", torch.int32, (T, n + 1)), body("t", torch.int32, (T, 2 * cap, 3)),
            body("toff", torch.int32, (T, n + 1)))


def test_chains_with_the_other_stages(ring_fusion):
    """simplify(0.05) -> fragments -> normals, each against its restatement on what the stage before left; then fragments -> simplify."""
    import torch
    _, fus = ring_fusion
    plan, n, cap = fus.plan, fus.n_maps, fus.capacity
    out_s, refs_s = simplify_cases.check_device(torch, plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, 0.05)
    out_f, refs_f = check_device(torch, plan, *_simplified(torch, out_s, 1, n, cap), 20)
    assert 0 < refs_f[0]["removed_vertices"] < refs_s[0]["cells"] and len(refs_f[0]["triangles"]) > 0
    _, refs_n = normals_cases.check_device(torch, plan, *out_f.tensors(torch))
    assert refs_n[0]["used"] > 0 and refs_n[0]["used"] + refs_n[0]["skipped"] == len(refs_f[0]["triangles"])
    out_f, refs_f = _check_fusion(fus, 64)
    _, refs_s = simplify_cases.check_device(torch, plan, *out_f.tensors(torch), 0.05)
    assert 0 < refs_s[0]["cells"] < len(refs_f[0]["vertices"])


def test_scratch_reuse_in_both_orders(gpu):
    """The parents and the sizes are reserved by the first call that filters: "off" first and the filter behind it, and the other way
    round, on plans of their own.  (A plan's tick count is fixed; a larger batch behind a smaller one is test_host_exports' second mesh.)"""
    import torch
    case = CASES["ticks"]
    for order in ((1, 2, 1, 600), (600, 1, 2)):
        c = clouds(torch, case)
        try:
            for m in order:
                check_device(torch, c.plan, c.v, c.off, c.t, c.toff, m)
        finally:
            c.close()


def _restated(v, t, m, cell):
    r = fragments_ref.fragments(v, [0, len(v)], t, [0, len(t)], m)
    rv, rt = r["vertices"], r["triangles"]
    if cell > 0 and len(rv):
        s = simplify_ref.simplify(rv, [0, len(rv)], rt if len(rt) else None, [0, len(rt)], cell)
        rv, rt = s["vertices"], (s["triangles"] if len(rt) else rt)
    return rv, rt


def test_host_exports(gpu, orc):
    """After a merge call: open, fragments, lod if cell > 0, normals if asked, pack -- against the restatements' chain through the oracle's
    packers and the numpy PLY-with-normals packer."""
    from tests.test_normals_gpu import ply_with_normals
    L = native.lib()
    small_rig = color_cases.ring(4, sizes=[(64, 48)] * 4)
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    for this, n_vertices, settings in ((small_rig, 6084, ((64, 0.0),)), (rig, 11087, ((256, 0.0), (2, 0.05), (64, 0.2), (2 ** 31 - 1, 0.0), (20000, 0.05)))):
        v, t, err = export(this)                          # the second mesh is the larger one: the context's scratch grows
        assert err == "" and len(v) == n_vertices and len(t) > 0
        plain = native.last_mesh_transfer_frame(), native.last_mesh_ply()
        for m, cell in settings:
            rv, rt = _restated(v, t, m, cell)
            assert native.last_mesh_transfer_frame_fragments(m, cell) == orc.transfer_frame(rv, rt), (m, cell)
            assert native.last_mesh_ply_fragments(m, cell) == orc.ply_binary(rv, rt), (m, cell)
            nrm = normals_ref.normals(rv, [0, len(rv)], rt, [0, len(rt)])["normals"] if len(rv) else np.zeros((0, 3), np.float32)
            assert native.last_mesh_ply_fragments(m, cell, with_normals=True) == ply_with_normals(rv, nrm, rt), (m, cell)
            assert len(rv) < len(v)
        assert len(_restated(v, t, 2 ** 31 - 1, 0.0)[0]) == 0
        # off: the plain exports byte for byte
        for m in (1, 0, -5):
            for cell in (0.0, -1.0, float("nan")):
                assert (native.last_mesh_transfer_frame_fragments(m, cell), native.last_mesh_ply_fragments(m, cell)) == plain, (m, cell)
        assert native.last_mesh_ply_fragments(1, 0.0, with_normals=True) == native.last_mesh_ply_normals(0.0)
        assert native.last_mesh_ply_fragments(1, 0.05) == native.last_mesh_ply_lod(0.05)
        # out == NULL: the bound of the unfiltered mesh
        assert L.lsnLastMeshTransferFrameFragments(256, 0.0, None, 0) >= len(plain[0])
        assert L.lsnLastMeshPlyFragments(256, 0.0, 0, None, 0) == len(plain[1]) == native.ply_binary_bytes(len(v), len(t))
        assert L.lsnLastMeshPlyFragments(256, 0.0, 1, None, 0) == native.ply_normals_bytes(len(v), len(t))
        small = np.zeros(100, np.uint8)
        assert L.lsnLastMeshPlyFragments(256, 0.0, 0, small.ctypes.data, 100) == -1 and "buffer holds" in native.last_error()
        assert L.lsnLastMeshTransferFrameFragments(256, 0.0, small.ctypes.data, 100) == -1 and "buffer holds" in native.last_error()
        # the resident mesh is as it was
        assert (native.last_mesh_transfer_frame(), native.last_mesh_ply()) == plain
    # a resident cloud without triangles: off copies, the filter and the normals are refused
    rig1 = color_cases.ring(1, sizes=[(64, 48)], of=3)
    native.generate_vertices_from_depth_map(rig1.depth_maps, rig1.depth_colors, rig1.widths, rig1.heights, rig1.intr, rig1.wt, rig1.bounds, 0)
    assert native.last_mesh_ply_fragments(1, 0.0) == native.last_mesh_ply()
    with pytest.raises(native.NativeUtilsError, match="d_triangles is null"):
        native.last_mesh_ply_fragments(2, 0.0)
    with pytest.raises(native.NativeUtilsError, match="no triangles"):
        native.last_mesh_ply_fragments(1, 0.0, with_normals=True)


def test_stream_example_with_min_fragment(gpu, tmp_path):
    """examples/stream --min-fragment N: stream and PLY go through the filter -- fewer vertices than without, the file as long as its
    header says, the same tick count."""
    import os
    import subprocess
    from livescan3d_amd import synth
    from tests.support import ROOT
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples"), "stream"], stdout=subprocess.DEVNULL)
    n, w, h = 2, 96, 80
    rig = synth.make_rig("scene", n, w, h, seed=21, bounds=synth.CROP_BOUNDS)
    recs = []
    for i in range(n):
        depth = rig.depth_maps.view(np.uint16)[i * w * h:(i + 1) * w * h].reshape(h, w)
        rgb = rig.depth_colors[3 * i * w * h:3 * (i + 1) * w * h].reshape(h, w, 3)
        path = tmp_path / f"rec{i}.bin"
        path.write_bytes(native.recording_append(native.frame_encode(depth, rgb, None, 0), 0))
        recs.append(str(path))
    calib = np.concatenate([np.concatenate([rig.intr[7 * i:7 * i + 7], rig.wt[12 * i:12 * i + 12]]) for i in range(n)]).astype(np.float32)
    (tmp_path / "calib.bin").write_bytes(calib.tobytes())
    counts, wire = [], []
    for extra in ([], ["--min-fragment", "1"], ["--min-fragment", "64"], ["--min-fragment", "64", "--normals"]):
        out = subprocess.run([os.path.join(ROOT, "examples", "stream"), "--calib", str(tmp_path / "calib.bin"), "--bounds",
                              *[str(float(x)) for x in synth.CROP_BOUNDS], *extra, "--frames-out", str(tmp_path / "frames.bin"), "--ply",
                              str(tmp_path / "mesh.ply"), *recs], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "1 ticks" in out.stdout, out.stdout + out.stderr
        blob = (tmp_path / "mesh.ply").read_bytes()
        end = blob.index(b"end_header\n") + len(b"end_header\n")
        lines = blob[:end].decode().split("\n")
        nv, nt = int(lines[2].split()[-1]), int([x for x in lines if x.startswith("element face")][0].split()[-1])
        assert len(blob) == (native.ply_normals_bytes(nv, nt) if "--normals" in extra else native.ply_binary_bytes(nv, nt))
        counts.append((nv, nt))
        wire.append((tmp_path / "frames.bin").read_bytes())
    assert counts[1] == counts[0] and wire[1] == wire[0]                     # off: what it always was
    assert 100 < counts[2][0] < counts[0][0] and 100 < counts[2][1] <= counts[0][1] and len(wire[2]) < len(wire[0])
    assert counts[3] == counts[2] and wire[3] == wire[2]
