"""lsnRefineFromDepthMaps / lsnRefineVertices / lsnRefineRelease on the GPU: the one call against the path it replaces
(generateVerticesFromDepthMap x n -> XYZ on the host -> lsnRefine) byte for byte, against the oracle, and its corner cases."""
import ctypes as C

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import color_cases, refine_ref, support

pytestmark = pytest.mark.gpu

TOL = 1e-4          # tests/test_icp_gpu.py's: the oracle's ICP against the device's, on every vertex, R and t
ITERS = (2, 5)
EMPTIES_SENSOR_0 = np.array([-0.45, -0.5, 0.2, 1.5, 1.5, 1.5], dtype=np.float32)   # behind the sphere, beside the far box: sensor 0 sees none of it


def _xyz(v):
    return np.stack([v["X"], v["Y"], v["Z"]], axis=1).astype(np.float32)


def _frames(rig, depth_maps=None, depth_colors=None):
    return (rig.depth_maps if depth_maps is None else depth_maps, rig.depth_colors if depth_colors is None else depth_colors,
            rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)


def _world(rig):
    wt = rig.wt.reshape(-1, 12)
    return wt[:, 3:].reshape(-1, 3, 3).copy(), wt[:, :3].copy()


def _pack(world_R, world_t):
    return np.concatenate([world_t.reshape(-1, 3), world_R.reshape(-1, 9)], axis=1).astype(np.float32).reshape(-1)


def _two_step(rig, iters=ITERS, outlier_filter=None, depth_maps=None, depth_colors=None):
    """The path the one call replaces, through the existing exports: generateVerticesFromDepthMap per sensor, X, Y, Z stripped on the host
    (MainWindowForm.cs:318-327), lsnRefine.  Returns the dict native.refine_frames returns (without the camera poses) and the blocks."""
    blocks = [native.generate_vertices_from_depth_map(*_frames(rig, depth_maps, depth_colors), i, outlier_filter=outlier_filter)
              for i in range(rig.n)]
    wR, wt = _world(rig)
    clouds, wR, wt, Rs, Ts = native.refine([_xyz(b) for b in blocks], wR, wt, *iters)
    return {"clouds": clouds, "counts": np.array([len(b) for b in blocks], np.int32), "Rs": Rs, "Ts": Ts, "wt": _pack(wR, wt)}, blocks


def _assert_same(got, want):
    assert np.array_equal(got["counts"], want["counts"]), (got["counts"], want["counts"])
    for key in ("Rs", "Ts", "wt"):
        assert got[key].tobytes() == want[key].tobytes(), key
    for i, (g, w) in enumerate(zip(got["clouds"], want["clouds"])):
        assert g.tobytes() == w.tobytes(), f"cloud {i}"


_CACHE = {}


def _rig3():
    if "rig3" not in _CACHE:
        _CACHE["rig3"] = synth.make_rig("scene", 3, 96, 80, seed=4, perturb=True)
    return _CACHE["rig3"]


def _rig3_two_step():
    if "two" not in _CACHE:
        _CACHE["two"] = _two_step(_rig3())
    return _CACHE["two"]


def _moved(got, blocks):
    return max(float(np.abs(g - _xyz(b)).max()) for g, b in zip(got["clouds"], blocks))


def test_one_call_equals_the_path_it_replaces(gpu):
    rig = _rig3()
    want, blocks = _rig3_two_step()
    assert list(want["counts"]) == [3818, 3465, 3791]      # odd sizes: the sensor blocks start off every vector width
    got = native.refine_frames(*_frames(rig), *ITERS)
    print("moved by", _moved(got, blocks), "m; Ts", got["Ts"].ravel())
    _assert_same(got, want)
    assert _moved(got, blocks) > 1e-3                       # the pass did move the clouds
    assert got["camera_R"] is None and got["camera_t"] is None


@pytest.mark.parametrize("flying", [None, (1, 20)], ids=["plain", "flying-pixels"])
def test_correct_radial_equals_the_radial_export_then_the_call(gpu, flying):
    rig = _rig3()
    before = rig.depth_maps.copy(), rig.depth_colors.copy()
    setting = native.set_flying_pixel_filter(0, 0)
    native.set_flying_pixel_filter(*setting)
    dm, dc = native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, flying_pixels=flying)
    assert not np.array_equal(dm, rig.depth_maps)
    want = native.refine_frames(*_frames(rig, dm, dc), *ITERS)
    got = native.refine_frames(*_frames(rig), *ITERS, correct_radial=True, flying_pixels=flying)
    _assert_same(got, want)
    if flying is not None:      # the filter did something, and the setting is back where it was
        plain = native.refine_frames(*_frames(rig), *ITERS, correct_radial=True)
        assert not np.array_equal(plain["counts"], got["counts"]) or plain["clouds"][0].tobytes() != got["clouds"][0].tobytes()
        again = native.set_flying_pixel_filter(*setting)
        assert again == setting
    assert np.array_equal(rig.depth_maps, before[0]) and np.array_equal(rig.depth_colors, before[1])   # the caller's frames are never written


def test_outlier_switch_equals_the_two_step_path_with_the_switch_on(gpu):
    rig = _rig3()
    setting = native.set_outlier_filter(0, 0.0)
    native.set_outlier_filter(*setting)
    want, _ = _two_step(rig, outlier_filter=(10, 0.1))
    got = native.refine_frames(*_frames(rig), *ITERS, outlier_filter=(10, 0.1))
    print("counts with the filter", got["counts"], "without", _rig3_two_step()[0]["counts"])
    _assert_same(got, want)
    assert got["counts"].sum() < _rig3_two_step()[0]["counts"].sum()      # the filter removed vertices
    assert native.set_outlier_filter(*setting) == setting


def test_against_the_oracle(gpu, orc):
    rig = synth.make_rig("scene", 4, 256, 212, seed=7, perturb=True)
    n = rig.n
    v, counts = orc.generate_mesh_vertices(*_frames(rig))
    edges = np.concatenate([[0], np.cumsum(counts)])
    clouds = [_xyz(v[edges[i]:edges[i + 1]]) for i in range(n)]
    wR, wt = _world(rig)
    rng = np.random.default_rng(11)
    cR = np.stack([synth.rot_y(0.2 * i) @ synth.rot_x(0.3 * i) for i in range(n)]).astype(np.float32)
    ct = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    ref_c, ref_R, ref_t, ref_Rs, ref_Ts = orc.refine(clouds, wR, wt, *ITERS, n_threads=8)
    got = native.refine_frames(*_frames(rig), *ITERS, camera_R=cR, camera_t=ct)
    assert np.array_equal(got["counts"], counts[:n])
    errs = {"clouds": max(float(np.abs(g - r).max()) for g, r in zip(got["clouds"], ref_c)),
            "Rs": float(np.abs(got["Rs"] - ref_Rs).max()), "Ts": float(np.abs(got["Ts"] - ref_Ts).max()),
            "world": float(np.abs(got["wt"] - _pack(ref_R, ref_t)).max())}
    _, _, want_cR, want_ct = refine_ref.compose_poses(ref_Rs, ref_Ts, wR, wt, cR, ct)
    errs["camera"] = max(float(np.abs(got["camera_R"] - want_cR).max()), float(np.abs(got["camera_t"] - want_ct).max()))
    print(errs)
    assert all(e <= TOL for e in errs.values()), errs
    assert max(float(np.abs(g - c).max()) for g, c in zip(got["clouds"], clouds)) > 1e-4      # the clouds did move


def _assert_not_run(got, rig, blocks, cR, ct):
    n = rig.n
    assert np.array_equal(got["Rs"], np.broadcast_to(np.eye(3, dtype=np.float32), (n, 3, 3))) and not got["Ts"].any()
    wR, wt = _world(rig)
    want = refine_ref.compose_poses(got["Rs"], got["Ts"], wR, wt, cR, ct)
    assert got["wt"].tobytes() == _pack(want[0], want[1]).tobytes()
    assert got["camera_R"].tobytes() == want[2].tobytes() and got["camera_t"].tobytes() == want[3].tobytes()
    assert list(got["counts"]) == [len(b) for b in blocks]
    for g, b in zip(got["clouds"], blocks):
        assert g.tobytes() == _xyz(b).tobytes()


def test_not_runnable_passes_return_the_clouds_unrefined(gpu):
    rng = np.random.default_rng(2)
    cR, ct = rng.uniform(-1, 1, size=(3, 3, 3)).astype(np.float32), rng.uniform(-1, 1, size=(3, 3)).astype(np.float32)
    # a crop box that empties one sensor
    rig = synth.make_rig("scene", 3, 96, 80, seed=4, perturb=True, bounds=EMPTIES_SENSOR_0)
    blocks = [native.generate_vertices_from_depth_map(*_frames(rig), i) for i in range(3)]
    assert len(blocks[0]) == 0 and len(blocks[1]) > 0 and len(blocks[2]) > 0
    _assert_not_run(native.refine_frames(*_frames(rig), *ITERS, camera_R=cR, camera_t=ct), rig, blocks, cR, ct)
    # no passes asked for
    rig, (_, blocks) = _rig3(), _rig3_two_step()
    _assert_not_run(native.refine_frames(*_frames(rig), 0, 5, camera_R=cR, camera_t=ct), rig, blocks, cR, ct)
    _assert_not_run(native.refine_frames(*_frames(rig), 2, 0, camera_R=cR, camera_t=ct), rig, blocks, cR, ct)
    # one sensor
    one = synth.make_rig("scene", 1, 96, 80, seed=4)
    blocks = [native.generate_vertices_from_depth_map(*_frames(one), 0)]
    _assert_not_run(native.refine_frames(*_frames(one), *ITERS, camera_R=cR[:1], camera_t=ct[:1]), one, blocks, cR[:1], ct[:1])


def test_mixed_sizes_with_a_one_pixel_sensor(gpu):
    rig = color_cases.ring(3, sizes=[(64, 53), (1, 1), (41, 30)], seed=4, gains=False)
    want, _ = _two_step(rig)
    got = native.refine_frames(*_frames(rig), *ITERS)
    print("counts", got["counts"])
    _assert_same(got, want)


def test_null_frames_fail_and_touch_nothing(gpu):
    rig = _rig3()
    n = rig.n
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    outs = [np.full(k * n, 7.5, np.float32) for k in (12, 9, 3, 9, 3, 3 * 96 * 80)] + [np.full(n, 75, np.int32)]
    rc = native.lib().lsnRefineFromDepthMaps(n, None, p(rig.depth_colors), p(rig.widths), p(rig.heights), p(rig.intr), p(rig.wt),
                                             *[float(x) for x in rig.bounds], 0, 2, 5, *[p(a) for a in outs])
    assert rc == -1 and "bad arguments" in native.last_error()
    assert all((a == (75 if a.dtype == np.int32 else 7.5)).all() for a in outs)


def test_device_resident_tick(gpu):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rigs = [synth.make_rig("scene", 3, 64, 53, seed=s, perturb=True) for s in (1, 2, 3)]
    for r in rigs[1:]:      # one calibration per plan (DeviceFusion.from_rigs)
        assert np.array_equal(r.wt, rigs[0].wt) and np.array_equal(r.intr, rigs[0].intr)
    want = native.refine_frames(*_frames(rigs[1]), *ITERS)
    rng = np.random.default_rng(3)
    cR, ct = rng.uniform(-1, 1, size=(3, 3, 3)).astype(np.float32), rng.uniform(-1, 1, size=(3, 3)).astype(np.float32)
    with DeviceFusion.from_rigs(rigs) as fusion:
        fusion.run()
        offsets = fusion.host_offsets()
        assert list(np.diff(offsets[1])) == list(want["counts"])
        vertices_before, offsets_before = fusion.vertices.clone(), fusion.offsets.clone()
        total = int(offsets[1, -1])
        out = support.Guarded(torch, total * 12, gpu)
        wR, wt = _world(rigs[1])
        got_wR, got_wt, got_cR, got_ct, Rs, Ts = fusion.refine(1, *ITERS, world_R=wR, world_t=wt, camera_R=cR, camera_t=ct,
                                                               clouds_out=out.body())
        torch.cuda.synchronize()
        assert out.intact()
        clouds = out.body().cpu().numpy().view(np.float32).reshape(-1, 3)
        assert clouds.tobytes() == np.concatenate(want["clouds"]).tobytes()
        assert Rs.tobytes() == want["Rs"].tobytes() and Ts.tobytes() == want["Ts"].tobytes()
        assert _pack(got_wR, got_wt).tobytes() == want["wt"].tobytes()
        ref = refine_ref.compose_poses(Rs, Ts, wR, wt, cR, ct)
        assert got_cR.tobytes() == ref[2].tobytes() and got_ct.tobytes() == ref[3].tobytes()
        # the inputs are read only: tick 1's cloud and offsets as they were, ticks 0 and 2 untouched
        assert torch.equal(fusion.vertices, vertices_before) and torch.equal(fusion.offsets, offsets_before)
        # without the output buffer the poses are the same
        assert fusion.refine(1, *ITERS)[4].tobytes() == Rs.tobytes()


def test_release_frees_the_kept_state_and_the_next_pass_gives_the_same_bytes(gpu):
    rig = _rig3()
    first = native.refine_frames(*_frames(rig), *ITERS)
    total = int(first["counts"].sum())
    released = native.refine_release(0)
    print("released", released, "bytes for", total, "points")
    assert released >= 2 * 12 * total       # the issue's floor (the workspace alone clears it on a rig this small; the exact check is below)
    assert native.refine_release(0) == 0 and native.refine_release(-1) == 0
    _assert_same(native.refine_frames(*_frames(rig), *ITERS), first)
    assert native.refine_release(-1) > 0
    # a pass with nothing to refine keeps the clouds alone (no workspace, no "others", no seeds): 12 bytes per point, to the byte
    native.refine_frames(*_frames(rig), 0, 5)
    assert native.refine_release(0) == 12 * total


def test_lsn_refine_composes_through_the_one_composition(gpu):
    want, blocks = _rig3_two_step()
    wR, wt = _world(_rig3())
    got_R, got_t, _, _ = native.compose_poses(want["Rs"], want["Ts"], wR, wt)
    assert _pack(got_R, got_t).tobytes() == want["wt"].tobytes()
    assert np.abs(want["Ts"]).max() > 0
