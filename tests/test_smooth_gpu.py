"""lsnFusionSmooth / lsnFusionSmoothDiagnostics / lsnLastMeshPlySmooth / lsnLastMeshTransferFrameSmooth on the GPU against the CPU
restatement (tests/smooth_ref.py).

Bar: bit-exact -- the vertices of every tick equal the restatement's byte for byte and the diagnostics' four counts are equal; the output
lies between guard bands in a buffer prefilled with 249, nothing behind a tick's nVertices is written and the inputs are unchanged
(tests/smooth_cases.py check_device).  Every test fails without the feature (the exports are missing)."""
import os
import re

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, fragments_ref, merge_cases, normals_ref, simplify_ref, smooth_ref
from tests.smooth_cases import PREFILL, TAUBIN, Clouds, cases, check_device
from tests.simplify_ref import cloud
from tests.support import ROOT, Guarded, export

pytestmark = pytest.mark.gpu


def _check(c, *params, **kw):
    return check_device(c.torch, c.plan, c.v, c.off, c.t, c.toff, *params, **kw)


def test_hand_made_meshes(gpu):
    """One 8 x 8 sensor (capacity 64 vertices / 128 triangles), a case per tick in one plan; what lies behind each tick's counts is
    garbage (0x5A vertices, -3 indices) and must not be read.  Every set of parameters the cases name runs over ALL the ticks; a case's
    witness is asked of the restatement under its own parameters."""
    import torch
    named = {k: c for k, c in cases().items() if k != "fan_300"}
    c = Clouds(torch, [case.tick() for case in named.values()])
    settings = sorted({(case.iterations, case.lam, case.mu, case.pin) for case in named.values()})
    assert len(settings) >= 6 and {s[0] for s in settings} >= {1, 64} and {s[2] for s in settings} >= {0.0} and {s[3] for s in settings} == {False, True}
    for s in settings:
        _, refs = _check(c, *s)
        for (name, case), r in zip(named.items(), refs):
            if (case.iterations, case.lam, case.mu, case.pin) == s:
                case.witness(r, case)
    c.close()


def test_fan_of_300_triangles(gpu):
    """302 vertices near +-4095 on a 20 x 16 sensor's plan (capacity 320 / 640): the hub's sums pass 2^53 and are odd -- the conversion
    to double and the division round."""
    import torch
    case = cases()["fan_300"]
    c = Clouds(torch, [case.tick()], sizes=((20, 16),))
    assert c.plan.capacity == 320
    _, refs = _check(c, case.iterations, case.lam, case.mu, case.pin)
    case.witness(refs[0], case)
    c.close()


def _random_tick(rng, nv, nt, off=None, toff=None, cap=None):
    """Random positions and random triples (a few out of range, one repeated, a NaN and an infinite coordinate), and a strip of grid
    triangles in front of them so that some vertices are closed."""
    cap = cap or nv
    tri = rng.integers(0, max(nv, 1), (nt, 3)).astype(np.int32)
    w = 8
    strip = [[i, i + 1, i + w] for r in range(3) for i in range(r * w, r * w + w - 1)] + [[i + 1, i + w + 1, i + w] for r in range(3) for i in range(r * w, r * w + w - 1)]
    k = min(len(strip), nt)
    tri[:k] = np.asarray(strip, np.int32)[:k]
    if nt > 60:
        tri[rng.integers(k, nt, 4), rng.integers(0, 3, 4)] = [-1, nv, 2 ** 30, -2 ** 31]
        tri[k + 1] = tri[k + 1, 0]
    xyz = rng.uniform(-2, 2, (cap, 3))
    if nv > 40:
        xyz[33, 0], xyz[37, 2] = np.nan, np.inf
    return cloud(xyz), np.array(off or [0, nv], np.int32), tri, np.array(toff or [0, nt], np.int32)


def test_counts_around_the_workgroup_size(gpu):
    """255 / 256 / 257 vertices and 511 / 512 / 513 triangles on the 20 x 16 plan: the last lanes of a wave, a workgroup and the next."""
    import torch
    rng = np.random.default_rng(11)
    c = Clouds(torch, [_random_tick(rng, 255, 511), _random_tick(rng, 256, 512), _random_tick(rng, 257, 513), _random_tick(rng, 257, 255)], sizes=((20, 16),))
    _, refs = _check(c, 3, 0.5, -0.53, True)
    assert [len(r["vertices"]) for r in refs] == [255, 256, 257, 257] and [r["used"] + r["skipped"] for r in refs] == [511, 512, 513, 255]
    assert all(r["used"] > 100 and r["skipped"] >= 3 and 0 < r["pinned"] for r in refs)
    _check(c, 2, 1.0, 0.0, False)
    c.close()


def test_full_capacity_empty_and_clipped_ticks(gpu):
    """64 vertices and 128 triangles, the whole capacity; an empty tick between two full ones; a tick whose d_offsets[n_maps] and
    d_tri_offsets[n_maps] exceed the capacities (clipped); negative counts."""
    import torch
    rng = np.random.default_rng(5)
    ticks = [_random_tick(rng, 64, 128), (cloud(np.zeros((0, 3))), np.array([0, 0], np.int32), np.zeros((0, 3), np.int32), np.array([0, 0], np.int32)),
             _random_tick(rng, 64, 128), _random_tick(rng, 64, 128, off=[0, 64 + 5], toff=[0, 128 + 77]), _random_tick(rng, 64, 128, off=[0, -4], toff=[0, 128]),
             _random_tick(rng, 64, 128, off=[0, 64], toff=[3, -1]), _random_tick(rng, 61, 127)]
    c = Clouds(torch, ticks)
    _, refs = _check(c, 2, 0.5, -0.53, True)
    assert [len(r["vertices"]) for r in refs] == [64, 0, 64, 64, 0, 64, 61]
    assert [r["used"] + r["skipped"] for r in refs] == [128, 0, 128, 128, 128, 0, 127] and refs[4]["used"] == 0 and refs[5]["isolated"] == 64
    assert refs[0]["skipped"] >= 3 and refs[0]["used"] > 100
    c.close()


def test_the_grid_stride_loop_runs_twice(gpu):
    """More triangles than one trip of the scatter's (and the topology pass's) grid covers, on seven vertices: kSmMaxBlocks x kSmThreads
    + 300, read from the kernel's own constants; a 1056 x 1000 sensor's plan has room for them."""
    import torch
    src = open(os.path.join(ROOT, "livescan3d_amd", "csrc", "smooth.hip")).read()
    per_trip = int(re.search(r"kSmMaxBlocks = (\d+);", src).group(1)) * int(re.search(r"kSmThreads = (\d+);", src).group(1))
    nt = per_trip + 300
    rng = np.random.default_rng(9)
    tri = rng.integers(0, 7, (nt, 3)).astype(np.int32)
    c = Clouds(torch, [(cloud(rng.uniform(-2, 2, (7, 3))), np.array([0, 7], np.int32), tri, np.array([0, nt], np.int32))], sizes=((1056, 1000),))
    assert 2 * c.plan.capacity >= nt > per_trip
    _, refs = _check(c, 1, 0.5, -0.53, True)
    assert refs[0]["used"] > per_trip // 2 and refs[0]["skipped"] > per_trip // 4
    c.close()


RINGS = {"3x96x80": lambda: color_cases.ring(3, sizes=[(96, 80)] * 3), "4x64x48": lambda: color_cases.ring(4, sizes=[(64, 48)] * 4)}


@pytest.fixture(scope="module", params=sorted(RINGS))
def ring_fusion(request, gpu):
    from livescan3d_amd.fusion import DeviceFusion
    rig = RINGS[request.param]()
    fus = DeviceFusion.from_rigs([rig])
    fus.run_mesh()
    yield rig, fus
    fus.close()


def _smoothed_and_ref(torch, fus, *batch):
    """DeviceFusion.smooth with the defaults on a batch of one tick (the fusion's own unless handed in) against the restatement."""
    v, off, t, toff = batch if batch else (fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets)
    out, refs = check_device(torch, fus.plan, v, off, t, toff, *TAUBIN, True)
    s = fus.smooth(*TAUBIN, True, *batch)
    torch.cuda.synchronize()
    nv = len(refs[0]["vertices"])
    assert s.dtype == torch.uint8 and tuple(s.shape) == (1, fus.capacity, 16) and s[0, :nv].cpu().numpy().tobytes() == refs[0]["vertices"].tobytes()
    assert batch or (s[0, nv:].cpu().numpy() == PREFILL).all()      # (the batch's own tensor has held a longer mesh by then)
    return s, refs[0]


def test_ring_plain_thin_method_and_twice_into_the_same_buffer(ring_fusion):
    """run_mesh -> smooth; a second call into the same buffer gives the same bytes (the sums are left cleared: nothing accumulates), and so
    does a call with other parameters in between; DeviceFusion.smooth returns the same vertices in the batch's own prefilled tensor."""
    import torch
    _, fus = ring_fusion
    out, refs = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, *TAUBIN, True)
    d = fus.plan.smooth_diagnostics(0)
    assert d["used"] > 5000 and d["skipped"] == 0 and 0 < d["pinned"] < len(refs[0]["vertices"]) and d["isolated"] > 0
    first = out.body().clone()
    check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, 1, 1.0, 0.0, False)
    check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, *TAUBIN, True, out=out, refs=refs)
    assert torch.equal(first, out.body())
    s, r = _smoothed_and_ref(torch, fus)
    assert fus.smooth(*TAUBIN) is s and r["vertices"].tobytes() != fus.tick_bytes(0).tobytes()
    check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, 3, 0.5, -0.53, False)


def test_ring_after_simplify_and_after_fragments(ring_fusion):
    """The outputs of simplify(0.05) -- no grid triangles any more, vertices used many times -- and of fragments(256)."""
    import torch
    _, fus = ring_fusion
    nv = int(fus.host_offsets()[0, -1])
    v, off, t, toff, _ = fus.simplify(0.05)
    _, r = _smoothed_and_ref(torch, fus, v, off, t, toff)
    assert 0 < len(r["vertices"]) < nv and r["skipped"] == 0 and r["used"] > 0
    v, off, t, toff, _, _ = fus.fragments(256)
    _, r = _smoothed_and_ref(torch, fus, v, off, t, toff)
    assert 0 < len(r["vertices"]) <= nv and r["used"] > 0


def test_normals_of_the_smoothed_mesh(ring_fusion):
    """normals() on the smoothed vertices equals normals_ref on the restated ones."""
    import torch
    _, fus = ring_fusion
    s, r = _smoothed_and_ref(torch, fus)
    n = fus.normals(vertices=s)
    torch.cuda.synchronize()
    want = normals_ref.normals(r["vertices"], fus.host_offsets()[0], fus.tick_triangles(0), fus.host_tri_offsets()[0])
    nv = len(r["vertices"])
    assert n[0, :nv].cpu().numpy().tobytes() == want["normals"].tobytes() and want["used"] > 5000
    plain = normals_ref.normals(fus.tick_cloud(0)[0], fus.host_offsets()[0], fus.tick_triangles(0), fus.host_tri_offsets()[0])
    assert plain["normals"].tobytes() != want["normals"].tobytes()


def test_after_overlay_merge(gpu):
    """The merge rewrites the triangles (the set-up of tests/test_simplify_gpu.py::test_after_overlay_merge)."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = merge_cases.wall(4, 96, 80)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        n_before = len(fus.tick_triangles(0))
        _, before = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, *TAUBIN, True)
        fus.overlay_merge()
        torch.cuda.synchronize()
        assert 0 < len(fus.tick_triangles(0)) < n_before
        _, after = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, *TAUBIN, True)
        assert 0 < after[0]["used"] and after[0]["used"] + after[0]["skipped"] == len(fus.tick_triangles(0))
        assert after[0]["vertices"].tobytes() != before[0]["vertices"].tobytes()


def test_a_second_plan_with_more_ticks(ring_fusion):
    """Three ticks of different frames, the middle one without valid depth, after the one-tick plan has run."""
    import copy
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rigs = [color_cases.ring(3, sizes=[(96, 80)] * 3, tick=k) for k in range(3)]
    rigs[1] = copy.copy(rigs[1])
    rigs[1].depth_maps = np.zeros_like(rigs[1].depth_maps)
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run_mesh()
        _, refs = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, 4, 0.5, -0.53, True)
        assert [len(r["vertices"]) > 10000 for r in refs] == [True, False, True] and len(refs[1]["vertices"]) == 0
        assert refs[0]["vertices"].tobytes() != refs[2]["vertices"].tobytes()
    _, fus1 = ring_fusion
    check_device(torch, fus1.plan, fus1.vertices, fus1.offsets, fus1.triangles, fus1.tri_offsets, 1, 0.5, -0.53, True)      # and the first plan still works


def test_refusals(ring_fusion):
    """A null argument, d_triangles == NULL, parameters out of range or NaN and an output that overlaps an input: -1, a message, and no
    output byte touched."""
    import torch
    _, fus = ring_fusion
    plan, cap = fus.plan, fus.capacity
    out = Guarded(torch, cap * 16, "cuda")
    out.body().fill_(PREFILL)
    before = fus.vertices.clone()
    good = {"v": fus.vertices.data_ptr(), "off": fus.offsets.data_ptr(), "t": fus.triangles.data_ptr(), "toff": fus.tri_offsets.data_ptr(), "out": out.ptr}

    def refused(msg, params=TAUBIN, **ptrs):
        a = dict(good, **ptrs)
        with pytest.raises(native.NativeUtilsError, match=msg):
            plan.smooth(*params, True, a["v"], a["off"], a["t"], a["toff"], a["out"])

    refused("null", v=0)
    refused("null", off=0)
    refused("null", toff=0)
    refused("null", out=0)
    refused("d_triangles", t=0)
    for it in (0, -1, 65):
        refused(r"iterations = -?\d+ is not in \[1, 64\]", (it, 0.5, -0.53))
    for lam in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        refused(r"lambda = \S+ is not in \(0, 1\]", (10, lam, -0.53))
    for mu in (0.1, -1.5, float("nan"), float("-inf")):
        refused(r"mu = \S+ is not in \[-1, 0\]", (10, 0.5, mu))
    refused("overlaps d_vertices", out=fus.vertices.data_ptr())
    refused("overlaps d_vertices", out=fus.vertices.data_ptr() + 16 * cap - 4)         # the last input bytes under the first output ones
    refused("overlaps d_vertices", v=out.ptr + 16 * cap - 4)
    refused("overlaps d_triangles", out=fus.triangles.data_ptr() + 12)
    refused("overlaps", out=fus.offsets.data_ptr())
    torch.cuda.synchronize()
    assert out.intact() and bool((out.body() == PREFILL).all().item()) and torch.equal(before, fus.vertices)
    L = native.lib()
    assert L.lsnFusionSmooth(None, 10, 0.5, -0.53, 1, good["v"], good["off"], good["t"], good["toff"], good["out"], None) == -1 and "null" in native.last_error()
    assert L.lsnFusionSmoothDiagnostics(None, 0, None, None, None, None, None) == -1
    fresh = native.FusionPlan(0, 1, [8], [8])
    with pytest.raises(native.NativeUtilsError, match="nothing has been smoothed"):
        fresh.smooth_diagnostics(0)
    fresh.close()
    plan.smooth(1, 1.0, -1.0, False, good["v"], good["off"], good["t"], good["toff"], good["out"])      # the ends of the ranges are inside
    with pytest.raises(native.NativeUtilsError, match="last call had 1 ticks"):
        plan.smooth_diagnostics(1)
    assert L.lsnFusionSmoothDiagnostics(plan._h, 0, None, None, None, None, None) == 0         # any pointer may be NULL


def _restated(v, t, min_vertices, cell, iterations, lam, mu, pin):
    """fragments -> level of detail -> smooth, each restatement on what the one before left."""
    r = fragments_ref.fragments(v, [0, len(v)], t, [0, len(t)], min_vertices)
    rv, rt = r["vertices"], r["triangles"]
    if cell > 0 and len(rv):
        s = simplify_ref.simplify(rv, [0, len(rv)], rt if len(rt) else None, [0, len(rt)], cell)
        rv, rt = s["vertices"], (s["triangles"] if len(rt) else rt)
    if iterations > 0:
        rv = smooth_ref.smooth(rv, [0, len(rv)], rt, [0, len(rt)], iterations, lam, mu, pin)["vertices"]
    return rv, rt


def test_last_mesh_exports(gpu, orc):
    """lsnLastMeshPlySmooth / lsnLastMeshTransferFrameSmooth on the resident mesh of the 3 x 96x80 ring: with iterations > 0 the PLY (with
    and without normals) and the frame packed from the restated vertices, alone and behind the fragment filter and the level of detail;
    with iterations = 0 the Fragments exports byte for byte; out == NULL: their bound; the refusals; the resident mesh unchanged."""
    from tests.test_normals_gpu import ply_with_normals
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    v, t, err = export(rig)
    assert err == "" and len(v) == 11087 and len(t) > 0
    plain = native.last_mesh_transfer_frame(), native.last_mesh_ply()
    for m, cell, pin in ((0, 0.0, True), (256, 0.0, False), (256, 0.05, True), (1, 0.05, True)):
        rv, rt = _restated(v, t, m, cell, *TAUBIN, pin)
        assert len(rv) > 1000 and (len(rv) < len(v)) == (m > 1 or cell > 0)
        assert native.last_mesh_transfer_frame_smooth(m, cell, *TAUBIN, pin) == orc.transfer_frame(rv, rt), (m, cell)
        assert native.last_mesh_ply_smooth(m, cell, *TAUBIN, pin) == orc.ply_binary(rv, rt), (m, cell)
        nrm = normals_ref.normals(rv, [0, len(rv)], rt, [0, len(rt)])["normals"]
        assert native.last_mesh_ply_smooth(m, cell, *TAUBIN, pin, with_normals=True) == ply_with_normals(rv, nrm, rt), (m, cell)
    for m, cell in ((0, 0.0), (256, 0.0), (256, 0.05), (1, 0.2)):
        for it in (0, -3):
            assert native.last_mesh_transfer_frame_smooth(m, cell, it, 0.5, -0.53) == native.last_mesh_transfer_frame_fragments(m, cell), (m, cell)
            assert native.last_mesh_ply_smooth(m, cell, it, float("nan"), 7.0) == native.last_mesh_ply_fragments(m, cell), (m, cell)
            assert native.last_mesh_ply_smooth(m, cell, it, 0.5, -0.53, with_normals=True) == native.last_mesh_ply_fragments(m, cell, with_normals=True)
    L = native.lib()
    assert L.lsnLastMeshTransferFrameSmooth(256, 0.0, 10, 0.5, -0.53, 1, None, 0) == L.lsnLastMeshTransferFrameFragments(256, 0.0, None, 0) >= len(plain[0])
    assert L.lsnLastMeshPlySmooth(256, 0.0, 10, 0.5, -0.53, 1, 0, None, 0) == len(plain[1])
    assert L.lsnLastMeshPlySmooth(256, 0.0, 10, 0.5, -0.53, 1, 1, None, 0) == native.ply_normals_bytes(len(v), len(t))
    small = np.zeros(100, np.uint8)
    assert L.lsnLastMeshPlySmooth(0, 0.0, 10, 0.5, -0.53, 1, 0, small.ctypes.data, 100) == -1 and "buffer holds" in native.last_error()
    with pytest.raises(native.NativeUtilsError, match="lambda"):
        native.last_mesh_ply_smooth(0, 0.0, 10, 0.0, -0.53)
    with pytest.raises(native.NativeUtilsError, match="iterations"):
        native.last_mesh_transfer_frame_smooth(0, 0.0, 65, 0.5, -0.53)
    assert (native.last_mesh_transfer_frame(), native.last_mesh_ply()) == plain
    # a resident cloud without triangles: off copies, the filter is refused
    rig1 = color_cases.ring(1, sizes=[(64, 48)], of=3)
    native.generate_vertices_from_depth_map(rig1.depth_maps, rig1.depth_colors, rig1.widths, rig1.heights, rig1.intr, rig1.wt, rig1.bounds, 0)
    assert native.last_mesh_ply_smooth(1, 0.0, 0) == native.last_mesh_ply()
    with pytest.raises(native.NativeUtilsError, match="no triangles"):
        native.last_mesh_ply_smooth(1, 0.0, 10)
    with pytest.raises(native.NativeUtilsError, match="no triangles"):
        native.last_mesh_transfer_frame_smooth(1, 0.0, 10)


def test_stream_example_smooths(gpu, tmp_path):
    """examples/stream --smooth 10,0.5,-0.53: the PLY has the plain run's header, colours and faces, and other positions; what goes on the
    wire has the plain run's length."""
    import subprocess
    from livescan3d_amd import synth
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
    blobs, lines = [], []
    for extra in ([], ["--smooth", "10,0.5,-0.53"]):
        out = subprocess.run([os.path.join(ROOT, "examples", "stream"), "--calib", str(tmp_path / "calib.bin"), "--bounds",
                              *[str(float(x)) for x in synth.CROP_BOUNDS], *extra, "--ply", str(tmp_path / "mesh.ply"), *recs],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "1 ticks" in out.stdout, out.stdout + out.stderr
        blobs.append((tmp_path / "mesh.ply").read_bytes())
        lines.append(out.stdout)
    assert lines[0] == lines[1] and len(blobs[0]) == len(blobs[1])
    end = blobs[0].index(b"end_header\n") + len(b"end_header\n")
    nv = int(blobs[0][:end].decode().split("\n")[2].split()[-1])
    rec = [np.frombuffer(b, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), nv, end) for b in blobs]
    assert nv > 100 and blobs[0][:end] == blobs[1][:end] and blobs[0][end + 15 * nv:] == blobs[1][end + 15 * nv:]
    assert np.array_equal(rec[0]["c"], rec[1]["c"]) and (rec[0]["p"] != rec[1]["p"]).any(axis=1).sum() > nv // 4
    assert np.abs(rec[0]["p"] - rec[1]["p"]).max() < 0.2
    bad = subprocess.run([os.path.join(ROOT, "examples", "stream"), "--calib", str(tmp_path / "calib.bin"), "--smooth", "10,2.0,-0.53", *recs],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 1 and "lambda" in bad.stderr
