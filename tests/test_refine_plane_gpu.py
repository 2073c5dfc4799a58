"""lsnRefineVerticesPlane (DeviceFusion.refine_plane): the point-to-plane refine pass on a resident tick with its vertex normals.

The one call against the sequence it stands for, issued here through the device exports -- per Gauss-Seidel step the two concatenations
(points and normals), IcpWorkspace.run_plane, the sensor's normals recomputed as n0 R in f32 -- byte for byte; its repeats (kept device
state, after lsnRefineRelease; the second pass of every call runs with seeds); and, on a room-corner rig whose sensor 1 is handed a
pose that is off by a known small motion, its residual to the cloud of the true poses against the point-to-point pass's on the same tick."""
import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import refine_ref, support

pytestmark = pytest.mark.gpu

F32 = np.float32
ITERS = (2, 5)


def _world(rig):
    wt = rig.wt.reshape(-1, 12)
    return wt[:, 3:].reshape(-1, 3, 3).copy(), wt[:, :3].copy()


@pytest.fixture(scope="module")
def tick(gpu):
    """The 3 x 96x80 scene rig of the refine tests through from_rigs -> run_mesh -> normals."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = synth.make_rig("scene", 3, 96, 80, seed=4, perturb=True)
    fus = DeviceFusion.from_rigs([rig])
    fus.run_mesh()
    normals = fus.normals()
    torch.cuda.synchronize()
    yield rig, fus, normals
    fus.close()
    native.refine_release(-1)


def _rotate32(n0, R):
    """n0 R for row vectors in f32, one rounding per operation, in apply_kernel's association."""
    n0, r = np.asarray(n0, F32), np.asarray(R, F32).ravel()
    out = np.empty_like(n0)
    for c in range(3):
        out[:, c] = (n0[:, 0] * r[c] + n0[:, 1] * r[3 + c]) + n0[:, 2] * r[6 + c]
    return out


def _sequence(torch, fus, normals, iters):
    """What the one call stands for, issued call by call.  Returns (clouds [total, 3], Rt [n, 12])."""
    n_refine, n_icp = iters
    off = fus.host_offsets()[0].astype(np.int64)
    n, total = fus.n_maps, int(off[-1])
    counts = np.diff(off)
    pts = fus.vertices[0, :total].view(torch.float32)[:, 1:4].contiguous()       # VertexC4ubV3f: four colour bytes, then X, Y, Z
    n0 = normals[0, :total].cpu().numpy()
    nrm = normals[0, :total].clone()
    Rt = torch.from_numpy(np.tile(np.concatenate([np.eye(3, dtype=F32).ravel(), np.zeros(3, F32)]), (n, 1))).cuda()
    st = int(torch.cuda.current_stream().cuda_stream)
    ws = native.IcpWorkspace(0, total - int(counts.min()), int(counts.max()))
    try:
        for _ in range(n_refine):
            for i in range(n):
                a, b = int(off[i]), int(off[i + 1])
                others = torch.cat([pts[:a], pts[b:]]).contiguous()
                others_n = torch.cat([nrm[:a], nrm[b:]]).contiguous()
                ws.run_plane(others.data_ptr(), others_n.data_ptr(), total - (b - a), pts.data_ptr() + 12 * a, b - a, Rt[i].data_ptr(),
                             Rt[i].data_ptr() + 36, n_icp, native.NN_GRID, st)
                torch.cuda.synchronize()
                nrm[a:b] = torch.from_numpy(_rotate32(n0[a:b], Rt[i, :9].cpu().numpy())).cuda()
        torch.cuda.synchronize()
        return pts.cpu().numpy(), Rt.cpu().numpy()
    finally:
        ws.close()


def _one_call(torch, gpu, fus, normals, rig, cR, ct, iters=ITERS):
    total = int(fus.host_offsets()[0, -1])
    out = support.Guarded(torch, total * 12, gpu)
    wR, wt = _world(rig)
    res = fus.refine_plane(0, normals, *iters, world_R=wR, world_t=wt, camera_R=cR, camera_t=ct, clouds_out=out.body())
    torch.cuda.synchronize()
    assert out.intact()
    return (out.body().cpu().numpy().view(F32).reshape(-1, 3),) + tuple(res)


def test_one_call_equals_the_sequence_it_stands_for(gpu, tick):
    import torch
    rig, fus, normals = tick
    diag = fus.plan.normals_diagnostics(0)
    assert diag["zero_normals"] > 0, diag                    # the skip rule is live: some matches meet a (0, 0, 0) normal
    vertices_before, normals_before = fus.vertices.clone(), normals.clone()
    rng = np.random.default_rng(3)
    cR, ct = rng.uniform(-1, 1, size=(3, 3, 3)).astype(F32), rng.uniform(-1, 1, size=(3, 3)).astype(F32)
    native.refine_release(-1)
    clouds, wR, wt, gcR, gct, Rs, Ts = _one_call(torch, gpu, fus, normals, rig, cR, ct)
    want_clouds, want_Rt = _sequence(torch, fus, normals, ITERS)
    assert clouds.tobytes() == want_clouds.tobytes()
    assert Rs.tobytes() == np.ascontiguousarray(want_Rt[:, :9]).tobytes() and Ts.tobytes() == np.ascontiguousarray(want_Rt[:, 9:]).tobytes()
    ref = refine_ref.compose_poses(Rs, Ts, *_world(rig), cR, ct)
    assert wR.tobytes() == ref[0].tobytes() and wt.tobytes() == ref[1].tobytes()
    assert gcR.tobytes() == ref[2].tobytes() and gct.tobytes() == ref[3].tobytes()
    moved = float(np.abs(clouds - fus.vertices[0, :len(clouds)].view(torch.float32)[:, 1:4].cpu().numpy()).max())
    print("moved by", moved, "m; Ts", Ts.ravel())
    assert moved > 1e-3 and np.abs(Ts).max() > 0
    # the inputs are read only
    assert torch.equal(fus.vertices, vertices_before) and torch.equal(normals.view(torch.uint8), normals_before.view(torch.uint8))
    # the point-to-point pass on the same tick is another result: the normals were used
    assert fus.refine(0, *ITERS)[4].tobytes() != Rs.tobytes()

    # again on the kept device state, after a release, and the release reports the three normals buffers with the rest
    again = _one_call(torch, gpu, fus, normals, rig, cR, ct)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (clouds, wR, wt, gcR, gct, Rs, Ts)))
    counts = np.diff(fus.host_offsets()[0])
    held_plane = native.refine_release(0)
    fus.refine(0, *ITERS)
    held_point = native.refine_release(0)
    assert held_plane - held_point == 12 * (3 * int(counts.sum()) - int(counts.min())), (held_plane, held_point)
    fresh = _one_call(torch, gpu, fus, normals, rig, cR, ct)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(fresh, (clouds, wR, wt, gcR, gct, Rs, Ts)))


def test_nothing_to_refine_and_bad_arguments(gpu, tick):
    import torch
    rig, fus, normals = tick
    eye = np.broadcast_to(np.eye(3, dtype=F32), (3, 3, 3))
    for iters in ((0, 5), (2, 0)):
        clouds, _, _, _, _, Rs, Ts = _one_call(torch, gpu, fus, normals, rig, None, None, iters)
        assert np.array_equal(Rs, eye) and not Ts.any()
        assert clouds.tobytes() == fus.vertices[0, :len(clouds)].view(torch.float32)[:, 1:4].cpu().numpy().tobytes()
    with pytest.raises(native.NativeUtilsError, match="lsnRefineVerticesPlane"):
        native.refine_vertices_plane(0, 3, fus.vertices[0].data_ptr(), None, fus.offsets[0].data_ptr(), *ITERS)


def _corner_rig(w, h, off_pose=None, azimuths=(25.0, 45.0, 65.0), pitch=20.0, radius=1.6):
    """Three sensors looking into a room corner (walls x = 0.9 and z = 0.9, floor y = -0.6) from nearby poses: every sensor sees all three
    planes, so the scene constrains all six degrees of freedom.  Ray-cast in float64 with synth.scene_frame's conventions, depth rounded
    to millimetres.  off_pose = (R, t): sensor 1 is HANDED a pose that is off by that motion (as synth.make_rig's perturb does); the
    frames are the same either way."""
    import math
    planes = [(np.array([1.0, 0, 0]), 0.9), (np.array([0, 0, 1.0]), 0.9), (np.array([0, -1.0, 0]), 0.6)]      # n . p = c, n pointing out of the room
    cx, cy, fx, fy = synth.kinect_intrinsics(w, h).astype(np.float64)[:4]
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack([(x - cx) / fx, (cy - y) / fy, np.ones_like(x)], axis=-1)
    depths, rgbs, intr, wt = [], [], [], []
    for s, az in enumerate(azimuths):
        R, t = synth.rot_y(math.radians(az)) @ synth.rot_x(math.radians(pitch)), np.array([0.0, 0.0, -radius])
        o, d = R @ t, dc @ R.T
        z = np.full((h, w), np.inf)
        for n, c in planes:
            nd = d @ n
            with np.errstate(divide="ignore", invalid="ignore"):
                hit = np.where(nd > 1e-9, (c - n @ o) / nd, np.inf)
            z = np.minimum(z, np.where(hit > 0, hit, np.inf))
        depth = np.where(np.isfinite(z), np.rint(1000.0 * np.where(np.isfinite(z), z, 0)), 0)
        depths.append(np.where((depth >= 500) & (depth <= 4500), depth, 0).astype(np.uint16))
        rgbs.append(np.full((h, w, 3), 128, np.uint8))
        intr.append(synth.kinect_intrinsics(w, h))
        if off_pose is not None and s == 1:
            R, t = R @ off_pose[0], t + off_pose[1]
        wt.append(synth.pack_pose(R, t))
    return synth.Rig(depths, rgbs, np.concatenate(intr), np.concatenate(wt), synth.DEFAULT_BOUNDS)


def _tick_cloud(torch, fus):
    total = int(fus.host_offsets()[0, -1])
    return fus.vertices[0, :total].view(torch.float32)[:, 1:4].cpu().numpy()


def test_plane_pass_undoes_a_known_motion_better(gpu):
    """A room-corner rig whose sensor 1 is handed a pose that is off by a known small motion (Ry(1 deg) Rx(0.5 deg), 1 cm -- what
    synth.make_rig's perturb applies): the residual to the cloud of the rig with the true poses, after the point-to-point pass and after
    the point-to-plane pass on the same tick.  Both are measured here; the demand is only that the second is the smaller."""
    import math
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    off = (synth.rot_y(math.radians(1.0)) @ synth.rot_x(math.radians(0.5)), np.array([0.01, -0.004, 0.007]))
    with DeviceFusion.from_rigs([_corner_rig(96, 80)]) as true_fus:
        true_fus.run_mesh()
        torch.cuda.synchronize()
        truth, true_offsets = _tick_cloud(torch, true_fus), true_fus.host_offsets()[0].copy()
    with DeviceFusion.from_rigs([_corner_rig(96, 80, off)]) as fus:
        fus.run_mesh()
        normals = fus.normals()
        torch.cuda.synchronize()
        assert np.array_equal(fus.host_offsets()[0], true_offsets) and fus.plan.normals_diagnostics(0)["zero_normals"] > 0
        start_cloud = _tick_cloud(torch, fus)
        total = len(truth)
        out_point, out_plane = torch.zeros((total, 3), dtype=torch.float32, device=gpu), torch.zeros((total, 3), dtype=torch.float32, device=gpu)
        fus.refine(0, 2, 10, clouds_out=out_point)
        fus.refine_plane(0, normals, 2, 10, clouds_out=out_plane)
        torch.cuda.synchronize()

        def residual(cloud):
            return float(np.linalg.norm(cloud.astype(np.float64) - truth, axis=1).mean())

        start, res_point, res_plane = residual(start_cloud), residual(out_point.cpu().numpy()), residual(out_plane.cpu().numpy())
        print(f"mean residual to the cloud of the true poses: {start:.3e} m at the start, {res_point:.3e} m after the point-to-point pass, "
              f"{res_plane:.3e} m after the point-to-plane pass")
        assert start > 5e-3 and res_plane < res_point, (start, res_point, res_plane)
    native.refine_release(-1)
