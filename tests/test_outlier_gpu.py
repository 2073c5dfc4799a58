"""The outlier filter (lsnSetOutlierFilter, lsnFusionOutlierFilter) on the GPU against the numpy restatement (tests/outlier_ref.py).

Bar: bit-exact -- a filtered single-sensor call equals filter() applied to the unfiltered cloud; a filtered merge call equals the same call
without the filter on the restatement's masked maps; the device-resident batch equals the exports."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, merge_cases, outlier_ref
from tests.support import ROOT, child

pytestmark = pytest.mark.gpu


def _rigs_small():
    return {"scene": synth.make_rig("scene", 4, 256, 212, seed=3),
            "ring": color_cases.ring(4, sizes=[(256, 212)] * 4, of=8),
            "wall": merge_cases.wall(4)}


def _verts(rig, i, setting=None):
    return native.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i,
                                                   outlier_filter=setting)


def _check_sensors(rig, k, d):
    removed = 0
    for i in range(rig.n):
        plain = _verts(rig, i)
        got = _verts(rig, i, (k, d))
        want = outlier_ref.filter_vertices(plain, k, d)
        assert got.tobytes() == want.tobytes(), (i, k, d, len(got), len(want))
        removed += len(plain) - len(want)
    return removed


@pytest.mark.parametrize("kind", ["scene", "ring", "wall"])
def test_single_sensor_export_is_filtered(gpu, kind):
    """Fails without the feature: generateVerticesFromDepthMap had no filter."""
    rig = _rigs_small()[kind]
    assert _check_sensors(rig, 10, 0.01) > 0
    _check_sensors(rig, 10, 0.1)


def test_tiny_frames_and_empty_sensor(gpu):
    for w, h in [(1, 1), (3, 2)]:
        rig = color_cases.ring(2, sizes=[(w, h)] * 2, bounds=color_cases.WIDE_BOUNDS, of=8)
        for k, d in [(1, 0.01), (2, 0.01), (6, 1e30), (6, 0.5)]:
            _check_sensors(rig, k, d)
    # a crop box that leaves sensor 0 without vertices
    rig = color_cases.ring(3, sizes=[(128, 106)] * 3, of=8)
    rig.bounds = np.array([-1.5, -1.0, -1.5, 1.5, 1.5, -1.4], dtype=np.float32)
    _check_sensors(rig, 10, 0.05)


def test_boundary_thresholds(gpu):
    """maxDist whose square equals a recorded kDistance, one float step either side; thr = inf and FLT_MAX; k = 1, 2, n, n + 1."""
    rig = color_cases.ring(1, sizes=[(48, 40)], bounds=color_cases.WIDE_BOUNDS, of=8)
    plain = _verts(rig, 0)
    n = len(plain)
    assert n > 20
    kd = outlier_ref.k_distance(plain, 10)
    base = float(np.sqrt(np.float64(np.median(kd))))
    cands = []
    for v in (np.float32(base), np.nextafter(np.float32(base), np.float32(0)), np.nextafter(np.float32(base), np.float32(1e9))):
        cands.append(float(v))
    cands += [float(np.sqrt(np.float64(FLT))) for FLT in [outlier_ref.FLT_MAX]] + [1e30]
    for k in (1, 2, 10, n, n + 1):
        for d in cands:
            got = _verts(rig, 0, (k, d))
            assert got.tobytes() == outlier_ref.filter_vertices(plain, k, d).tobytes(), (k, d)


def test_noop_settings_behave_like_the_reference(gpu):
    rig = _rigs_small()["scene"]
    plain = _verts(rig, 1)
    for k, d in [(0, 0.1), (-3, 0.1), (10, 0.0), (10, -1.0), (10, float("nan"))]:
        assert _verts(rig, 1, (k, d)).tobytes() == plain.tobytes()
    base = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    off = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                               outlier_filter=(0, 0.0))
    assert base[0].tobytes() == off[0].tobytes() and np.array_equal(base[1], off[1])


@pytest.mark.parametrize("flags", [(False, False), (True, False), (False, True), (True, True)])
def test_merge_call_is_the_call_on_masked_maps(gpu, orc, flags):
    rig = color_cases.ring(4, sizes=[(256, 212)] * 4, of=8)
    k, d = 10, 0.02
    masked, removed = outlier_ref.filter_rig(rig, k, d, orc)
    assert sum(int(r.sum()) for r in removed) > 0
    mr = outlier_ref.masked_rig(rig, masked)
    ct, tri = flags
    got = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                               color_transfer=ct, generate_triangles=tri, overlay_merge=True, outlier_filter=(k, d))
    want = native.generate_mesh_from_depth_maps(mr.depth_maps, mr.depth_colors, mr.widths, mr.heights, mr.intr, mr.wt, mr.bounds,
                                                color_transfer=ct, generate_triangles=tri, overlay_merge=True)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    if flags == (False, False):
        v, _, t = orc.generate_mesh(mr.depth_maps, mr.depth_colors, mr.widths, mr.heights, mr.intr, mr.wt, mr.bounds)
        assert got[0].tobytes() == v.tobytes() and np.array_equal(got[1], t)
        assert native.last_mesh_ply() == orc.ply_binary(got[0], got[1])   # lsnLastMesh* serve the filtered mesh


def test_correct_and_generate_mesh(gpu):
    rig = _rigs_small()["scene"]
    k, d = 10, 0.02
    v, t, dm, dc = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                    outlier_filter=(k, d))
    v0, t0, dm0, dc0 = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    assert dm.tobytes() == dm0.tobytes() and dc.tobytes() == dc0.tobytes()   # the corrected maps go back unmasked
    cr = outlier_ref.masked_rig(rig, dm0)
    cr.depth_colors = dc0
    want = native.generate_mesh_from_depth_maps(cr.depth_maps, cr.depth_colors, cr.widths, cr.heights, cr.intr, cr.wt, cr.bounds,
                                                outlier_filter=(k, d))
    assert v.tobytes() == want[0].tobytes() and np.array_equal(t, want[1])
    assert len(v) < len(v0)


def _device_batch(rigs, k, d, in_place):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs(rigs) as fus:
        out = fus.depth if in_place else torch.empty_like(fus.depth)
        fus.run()
        fus.outlier_filter(k, d, out)
        o = fus.host_offsets()
        diags = [fus.plan.outlier_diagnostics(t, int(o[t, -1])) for t in range(len(rigs))]
        fus.run_mesh(out)
        res = [(fus.tick_cloud(t)[0], fus.tick_triangles(t)) for t in range(len(rigs))]
        return res, diags, o, out.cpu().numpy()


def test_device_batch_equals_exports(gpu, orc):
    rigs = [color_cases.ring(4, sizes=[(256, 212)] * 4, of=8, tick=t) for t in range(16)]
    k, d = 10, 0.02
    res, diags, o, masked = _device_batch(rigs, k, d, in_place=False)
    res2, _, _, masked2 = _device_batch(rigs, k, d, in_place=True)
    assert masked.tobytes() == masked2.tobytes()
    for t, rig in enumerate(rigs):
        v, tris = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                       outlier_filter=(k, d))
        assert res[t][0].tobytes() == v.tobytes() and np.array_equal(res[t][1], tris), t
        assert res2[t][0].tobytes() == v.tobytes() and np.array_equal(res2[t][1], tris), t
        if t < 3:
            want_maps, removed = outlier_ref.filter_rig(rig, k, d, orc)
            assert masked[t].view(np.uint8).tobytes() == want_maps.tobytes()
            dg = diags[t]
            assert np.array_equal(dg["removed"].astype(bool), np.concatenate(removed))
            assert dg["removed_per_sensor"].tolist() == [int(r.sum()) for r in removed]
            assert dg["total"] == sum(int(r.sum()) for r in removed)
            counts = np.diff(o[t])
            assert dg["exact_per_sensor"].tolist() == [int(c) if c >= k else 0 for c in counts]


def test_grid_pass_both_outcomes(gpu):
    """k beyond what any small window holds, and a dense cluster close to the camera (many points per cell) beside sparse ones."""
    rig = synth.make_rig("scene", 2, 256, 212, seed=5)
    dm = rig.depth_maps.view("<u2").copy()
    dm[100 * 256 + 100:100 * 256 + 140] = 600    # a row of pixels 0.6 m from sensor 0
    rig.depth_maps = dm.view(np.uint8)
    rig.bounds = color_cases.WIDE_BOUNDS
    for k, d in [(60, 0.03), (200, 0.05), (3, 0.004)]:
        assert _check_sensors(rig, k, d) > 0


def test_full_size_exhaustive(gpu):
    """8 x 512x424 scene tick at (10, 0.01) and (10, 0.1): every removed vertex and 2000 random kept ones checked against their whole
    sensor block."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = synth.make_rig("scene", 8, 512, 424, seed=7)
    fus = DeviceFusion.from_rigs([rig])
    out = torch.empty_like(fus.depth)
    fus.run()
    v, o = fus.tick_cloud(0)
    rng = np.random.default_rng(3)
    for k, d in [(10, 0.01), (10, 0.1)]:
        fus.outlier_filter(k, d, out)
        dg = fus.plan.outlier_diagnostics(0, int(o[-1]))
        rem = dg["removed"].astype(bool)
        thr = outlier_ref.threshold(d)
        for s in range(rig.n):
            blk = outlier_ref.xyz(v[o[s]:o[s + 1]])
            r = rem[o[s]:o[s + 1]]
            bad = outlier_ref.neighbour_counts(blk, thr, np.flatnonzero(r))
            assert (bad < k).all(), (k, d, s)
            kept = np.flatnonzero(~r)
            sample = rng.choice(kept, size=min(2000, len(kept)), replace=False)
            assert (outlier_ref.neighbour_counts(blk, thr, sample) >= k).all(), (k, d, s)
        assert dg["total"] > 0 and dg["total"] < o[-1]
    fus.close()


DROP = ("LSN_OUTLIER_FILTER",)   # the children start without the switch of this shell


def test_environment_switch():
    # the child reads the switch by setting it and setting it back: nothing else runs in that process
    code = "from livescan3d_amd import native; p = native.set_outlier_filter(0, 0.0); native.set_outlier_filter(*p); print(p)"
    assert child(code, {}, drop=DROP)[0] == "(0, 0.0)"
    k, d = eval(child(code, {"LSN_OUTLIER_FILTER": "10,0.1"}, drop=DROP)[0])
    assert k == 10 and np.float32(d) == np.float32(0.1)
    assert child(code, {"LSN_OUTLIER_FILTER": "ten"}, drop=DROP)[0] == "(0, 0.0)"
    assert child(code, {"LSN_OUTLIER_FILTER": "10,0.1x"}, drop=DROP)[0] == "(0, 0.0)"


def test_environment_filters_the_exports_and_host_devices(gpu):
    """$LSN_OUTLIER_FILTER in a child process filters the merge call; with $LSN_HOST_DEVICES=0,0,0 the bytes are the same."""
    code = ("import hashlib, numpy as np; from livescan3d_amd import native, synth; "
            "r = synth.make_rig('scene', 4, 256, 212, seed=3); "
            "v, t = native.generate_mesh_from_depth_maps(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr, r.wt, r.bounds); "
            "print(len(v), hashlib.sha256(v.tobytes() + t.tobytes()).hexdigest())")
    rig = synth.make_rig("scene", 4, 256, 212, seed=3)
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                outlier_filter=(10, 0.02))
    import hashlib
    want = f"{len(v)} {hashlib.sha256(v.tobytes() + t.tobytes()).hexdigest()}"
    assert child(code, {"LSN_OUTLIER_FILTER": "10,0.02"}, drop=DROP)[0] == want
    assert child(code, {"LSN_OUTLIER_FILTER": "10,0.02", "LSN_HOST_DEVICES": "0,0,0"}, drop=DROP)[0] == want
    plain = child(code, {"LSN_HOST_DEVICES": "0,0,0"}, drop=DROP)[0]
    assert plain != want and int(plain.split()[0]) > len(v)


def test_device_filter_on_the_reference_fixture(gpu):
    """The kernels straight against the reference's own filter() (tests/golden/outlier_filter_ref.npz): every fixture cloud handed to
    lsnFusionOutlierFilter as a one-sensor cloud; the removed flags equal the reference's changedVerticesMap in every case."""
    import torch
    g = np.load(os.path.join(ROOT, "tests", "golden", "outlier_filter_ref.npz"))
    names = [str(x) for x in g["cloud_names"]]
    plans = {}
    n_cases = 0
    for c in range(len(g["case_k"])):
        name = names[int(g["case_cloud"][c])]
        pts = g[f"cloud_{name}"]
        k, d = int(g["case_k"][c]), float(g["case_max_dist"][c])
        n = len(pts)
        if name not in plans:
            w = 64
            h = (n + w - 1) // w
            plan = native.FusionPlan(0, 1, [w], [h])
            plan.set_params(synth.kinect_intrinsics(w, h), synth.pack_pose(np.eye(3), np.zeros(3)), color_cases.WIDE_BOUNDS)
            rec = np.zeros(plan.capacity, dtype=native.VERTEX_DTYPE)
            rec["X"][:n], rec["Y"][:n], rec["Z"][:n] = pts[:, 0], pts[:, 1], pts[:, 2]
            plans[name] = (plan, torch.zeros(w * h, dtype=torch.int16, device="cuda"),
                           torch.from_numpy(rec.view(np.uint8).copy()).cuda(), torch.tensor([0, n], dtype=torch.int32, device="cuda"))
        plan, depth, verts, off = plans[name]
        out = torch.empty_like(depth)
        plan.outlier_filter(k, d, depth.data_ptr(), verts.data_ptr(), off.data_ptr(), out.data_ptr())
        removed = plan.outlier_diagnostics(0, n)["removed"].astype(bool)
        changed = g[f"changed_{c}"]
        want = np.zeros(n, bool) if len(changed) == 0 else changed < 0
        assert np.array_equal(removed, want), (c, name, k, d)
        n_cases += 1
    for plan, *_ in plans.values():
        plan.close()
    assert n_cases == len(g["case_k"])


def test_tiny_radius_is_not_quadratic(gpu):
    """maxDist far below the point spacing (1e-12 m): the edge's floor keeps the cells small, the call is quick and exact."""
    import time
    rig = synth.make_rig("scene", 1, 512, 424, seed=5)
    plain = _verts(rig, 0)
    t0 = time.perf_counter()
    got = _verts(rig, 0, (2, 1e-12))
    assert time.perf_counter() - t0 < 5.0
    assert got.tobytes() == outlier_ref.filter_vertices(plain, 2, 1e-12).tobytes()
    assert len(got) < len(plain)
