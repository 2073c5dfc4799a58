"""Depth smoothing (depth_smooth.hip: lsnFusionSetDepthSmooth / lsnFusionDepthSmooth, lsnTickSetDepthSmooth, lsnSetDepthSmooth) on the GPU.

Bar: bit-exact against the numpy restatement (tests/depth_smooth_ref.py), with the tables the library itself returned
(lsnDepthSmoothGaussian) or hand-made ones; every flow that starts at raw frames equals the restatement chained with tests/flying_ref.py
and the existing oracle; with the switch off every flow returns the bytes it returns today.  Wherever a scene rig is compared, the
device's own diagnostics must first show that smoothing changed pixels of every sensor, so that no comparison is vacuous.
Every test here fails on a library without the feature (the exports do not exist)."""
import hashlib
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, depth_smooth_cases as cases, depth_smooth_ref as ref, flying_ref
from tests.support import Guarded, child

pytestmark = pytest.mark.gpu

FRAMES = [(1, 1), (8, 1), (7, 5), (128, 16), (136, 17), (264, 33)]       # w x h: below the window, one chunk, odd, one tile, tiles that end inside
WIDE = [(w, h) for w, h in FRAMES if w % 8 == 0]                         # every width a multiple of 8: the 16-byte form
SETTING = (2, 1.5, 12.0)


def _pack(frames):
    return np.concatenate([f.ravel() for f in frames]).astype("<u2")


class _Batch:
    """A plan of `sizes` sensors and T ticks with seeded noisy frames, its input at `shift` bytes behind a 16-byte boundary and its output
    between guard bands."""

    def __init__(self, sizes, T=2, shift=0, seed=0):
        import torch
        self.torch, self.sizes, self.T = torch, sizes, T
        self.plan = native.FusionPlan(0, T, [s[0] for s in sizes], [s[1] for s in sizes])
        self.frames = [[cases.frame(seed + 31 * t + i, w, h) for i, (w, h) in enumerate(sizes)] for t in range(T)]
        self.host = np.stack([_pack(row) for row in self.frames])
        self.nbytes = self.host.nbytes
        self.src = Guarded(torch, self.nbytes + shift, "cuda")
        self.src.body()[shift:].copy_(torch.from_numpy(self.host.view(np.uint8).ravel().copy()))
        self.src_ptr = self.src.ptr + shift
        self.dst = Guarded(torch, self.nbytes, "cuda")

    def run(self):
        self.dst.body().fill_(0x5A)
        self.plan.depth_smooth(self.src_ptr, self.dst.ptr)
        self.torch.cuda.synchronize()
        assert self.dst.intact() and self.src.intact()
        return self.dst.body().cpu().numpy().view("<u2").reshape(self.T, -1)

    def check(self, r, ws, wr, what):
        got = self.run()
        for t in range(self.T):
            want = [ref.smooth(f, r, ws, wr) for f in self.frames[t]]
            assert got[t].tobytes() == _pack(want).tobytes(), (what, t)
            ch, mv, total = self.plan.depth_smooth_diagnostics(t)
            cm = [ref.counts(f, o) for f, o in zip(self.frames[t], want)]
            assert ch.tolist() == [c[0] for c in cm] and mv.tolist() == [c[1] for c in cm] and total == sum(c[0] for c in cm), (what, t)


@pytest.mark.parametrize("form", ["wide", "odd_widths", "shifted"])
def test_kernels_equal_the_restatement(gpu, form):
    """Every frame size of the issue, two sensors and more of different sizes in one plan, two ticks, r = 1, 2, 3, the library's own
    Gaussian tables and random ones; the 16-byte form (widths that are multiples of 8, aligned buffers) and the element-wise form (an odd
    width in the plan; an input pointer 2 bytes off)."""
    b = _Batch(WIDE if form != "odd_widths" else FRAMES, shift=2 if form == "shifted" else 0, seed=11)
    rng = np.random.default_rng(5)
    for r, ss, sr in [(1, 1.0, 10.0), (2, 1.5, 12.0), (3, 2.0, 15.0)]:
        ws, wr = native.depth_smooth_gaussian(r, ss, sr)
        b.plan.set_depth_smooth(r, ws, wr)
        b.check(r, ws, wr, (form, r, "gaussian"))
        ch, _, total = b.plan.depth_smooth_diagnostics(0)
        assert total > 0 and (ch[2:] > 0).all()                   # not vacuous: the noise is smoothed in every frame beyond the tiny ones
        ws, wr = cases.random_tables(rng, r)
        b.plan.set_depth_smooth(r, ws, wr)
        b.check(r, ws, wr, (form, r, "random"))
    assert b.src.body().cpu().numpy()[b.src_ptr - b.src.ptr:].tobytes() == b.host.tobytes()      # the input stays as it was
    b.plan.close()


@pytest.mark.parametrize("case", cases.cases(), ids=[c.name for c in cases.cases()])
def test_hand_made_cases(gpu, case):
    import torch
    h, w = case.depth.shape
    plan = native.FusionPlan(0, 1, [w], [h])
    src = torch.from_numpy(case.depth.astype("<u2").view(np.int16).ravel().copy()).cuda()
    dst = Guarded(torch, 2 * w * h, "cuda")
    plan.set_depth_smooth(case.r, case.ws, case.wr)
    plan.depth_smooth(src.data_ptr(), dst.ptr)
    torch.cuda.synchronize()
    got = dst.body().cpu().numpy().view("<u2").reshape(h, w)
    want = case.want()
    assert np.array_equal(got, want), (case.name, got.tolist(), want.tolist())
    assert dst.intact()
    ch, mv, total = plan.depth_smooth_diagnostics(0)
    assert (int(ch[0]), int(mv[0])) == ref.counts(case.depth, want) and total == int(ch[0])
    plan.close()


def test_off_copies_and_refusals_change_nothing(gpu):
    import torch
    b = _Batch([(136, 17), (7, 5)], T=2, seed=3)
    plan = b.plan
    with pytest.raises(native.NativeUtilsError):
        plan.depth_smooth_diagnostics(0)                          # nothing has run yet
    assert b.run().tobytes() == b.host.tobytes()                  # off by default: the input's bytes
    assert plan.depth_smooth_diagnostics(1)[2] == 0
    ws, wr = native.depth_smooth_gaussian(*SETTING)
    plan.set_depth_smooth(SETTING[0], ws, wr)
    b.check(SETTING[0], ws, wr, "on")
    # every refused setting leaves the previous one in force
    bad_ws, bad_wr, no_centre, no_zero = ws.copy(), wr.copy(), ws.copy(), wr.copy()
    bad_ws[0, 1], bad_wr[3], no_centre[2, 2], no_zero[0] = 4096, 4096, 0, 0
    L = native.lib()
    for radius, s, q, n in [(4, ws, wr, wr.size), (2, bad_ws, wr, wr.size), (2, ws, bad_wr, wr.size), (2, no_centre, wr, wr.size),
                            (2, ws, no_zero, wr.size), (2, ws, wr, 0), (2, ws, wr, -1), (2, ws, np.zeros(1025, np.uint16) + 1, 1025),
                            (2, None, wr, wr.size), (2, ws, None, wr.size)]:
        sp = None if s is None else np.ascontiguousarray(s, np.uint16).ctypes.data
        qp = None if q is None else np.ascontiguousarray(q, np.uint16).ctypes.data
        assert L.lsnFusionSetDepthSmooth(plan._h, radius, sp, qp, n) == -1 and "lsnFusionSetDepthSmooth" in native.last_error(), (radius, n)
        b.check(SETTING[0], ws, wr, "after a refused setting")
    # an output that overlaps the input is refused with nothing written; so is a null argument
    before = b.src.buf.cpu().numpy().tobytes()
    for out in (b.src_ptr, b.src_ptr + 16, b.src_ptr + b.nbytes - 2):
        with pytest.raises(native.NativeUtilsError, match="overlap"):
            plan.depth_smooth(b.src_ptr, out)
    b.dst.body().fill_(0x5A)
    assert L.lsnFusionDepthSmooth(plan._h, None, b.dst.ptr, None) == -1 and L.lsnFusionDepthSmooth(plan._h, b.src_ptr, None, None) == -1
    torch.cuda.synchronize()
    assert b.src.buf.cpu().numpy().tobytes() == before and bool((b.dst.body() == 0x5A).all().item())
    b.check(SETTING[0], ws, wr, "after the refused calls")
    # the same tables again, other tables, off, on again
    plan.set_depth_smooth(SETTING[0], ws, wr)
    b.check(SETTING[0], ws, wr, "set again")
    ws3, wr3 = native.depth_smooth_gaussian(3, 2.0, 15.0)
    plan.set_depth_smooth(3, ws3, wr3)
    b.check(3, ws3, wr3, "replaced")
    plan.set_depth_smooth(0)
    assert b.run().tobytes() == b.host.tobytes() and plan.depth_smooth_diagnostics(0)[2] == 0
    plan.set_depth_smooth(-3, None, None)
    assert b.run().tobytes() == b.host.tobytes()
    plan.set_depth_smooth(1, *native.depth_smooth_gaussian(1, 1.0, 10.0))
    b.check(1, *native.depth_smooth_gaussian(1, 1.0, 10.0), "on again")
    plan.close()


# ---- the flows that start at raw frames ---------------------------------------------------------------------------------------------

def _ring(tick=0):
    return color_cases.ring(2, sizes=[(96, 80)] * 2, of=8, tick=tick)


def _want_tick(rig, orc, flying, smooth):
    """flying_ref, the restatement with the library's own tables, then the existing oracle: (maps in front of the correction, corrected
    maps, corrected colours, vertices, triangles).  Asserts that smoothing changed pixels of every sensor."""
    dm = rig.depth_maps
    if flying:
        dm, _ = flying_ref.filter_packed(dm, rig.widths, rig.heights, *flying)
    if smooth:
        ws, wr = native.depth_smooth_gaussian(*smooth)
        dm, changed, _ = ref.smooth_packed(dm, rig.widths, rig.heights, smooth[0], ws, wr)
        assert (changed > 0).all()
    cd, cc = orc.radial_correction(dm, rig.depth_colors, rig.widths, rig.heights, rig.intr)
    cd, cc = np.asarray(cd).view(np.uint8).ravel(), np.asarray(cc).ravel()
    v, _, t = orc.generate_mesh(cd, cc, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    return dm, cd, cc, v, t


@pytest.mark.parametrize("flying", [None, (1, 20)], ids=["smooth", "flying+smooth"])
def test_host_exports_smooth_between_filter_and_correction(gpu, orc, flying):
    rig = _ring()
    a = (rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr)
    _, cd, cc, v, t = _want_tick(rig, orc, flying, SETTING)
    _, pd, pc, pv, pt = _want_tick(rig, orc, flying, None)
    assert pd.tobytes() != cd.tobytes()
    gd, gc = native.radial_correction(*a, flying_pixels=flying, depth_smooth=SETTING)
    assert np.asarray(gd).view(np.uint8).tobytes() == cd.tobytes() and np.asarray(gc).tobytes() == cc.tobytes()
    for write_back in (True, False):
        gv, gt, gd, gc = native.correct_and_generate_mesh(*a, rig.wt, rig.bounds, write_back=write_back, flying_pixels=flying, depth_smooth=SETTING)
        assert gv.tobytes() == v.tobytes() and np.array_equal(gt, t)
        if write_back:
            assert np.asarray(gd).view(np.uint8).tobytes() == cd.tobytes() and np.asarray(gc).tobytes() == cc.tobytes()
        else:
            assert np.asarray(gd).view(np.uint8).tobytes() == rig.depth_maps.tobytes()
    # the switch was restored, radius 0 is off: today's bytes
    for kw in ({}, {"depth_smooth": (0, 1.5, 12.0)}):
        gd, gc = native.radial_correction(*a, flying_pixels=flying, **kw)
        assert np.asarray(gd).view(np.uint8).tobytes() == pd.tobytes() and np.asarray(gc).tobytes() == pc.tobytes()
        gv, gt, gd, gc = native.correct_and_generate_mesh(*a, rig.wt, rig.bounds, flying_pixels=flying, **kw)
        assert gv.tobytes() == pv.tobytes() and np.array_equal(gt, pt) and np.asarray(gd).view(np.uint8).tobytes() == pd.tobytes()
    assert native.set_depth_smooth(0) == (0, 0.0, 0.0)


CHILD = r"""
import hashlib
import numpy as np
from livescan3d_amd import native
from tests import color_cases
rig = color_cases.ring(2, sizes=[(96, 80)] * 2, of=8)
gd, gc = native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr)
v, t, d, c = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
mv, mt = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
sv = native.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, 1)
H = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()
print(H(np.asarray(gd).view(np.uint8), gc), H(v, np.asarray(t, np.int32), np.asarray(d).view(np.uint8), c), H(mv, np.asarray(mt, np.int32), sv))
"""

DROP = ("LSN_DEPTH_SMOOTH", "LSN_FLYING_PIXELS", "LSN_OUTLIER_FILTER", "LSN_HOST_PATH", "LSN_HOST_GROUP", "LSN_HOST_DEVICES")


def _H(*a):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()


@pytest.mark.parametrize("flow", [{}, {"LSN_HOST_GROUP": "1"}, {"LSN_HOST_DEVICES": "0,0"}], ids=["default", "group1", "shard2"])
def test_host_flows_with_the_environment_switches(gpu, orc, flow):
    """$LSN_DEPTH_SMOOTH with $LSN_FLYING_PIXELS in a child process: the one-device flow, a group per sensor, and the sharded flow with
    the one GPU listed twice.  The merge export and the single-sensor export do not smooth; with the switch unset every hash is today's."""
    rig = _ring()
    mv, _, mt = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    allv, counts = orc.generate_mesh_vertices(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    untouched = _H(mv, np.asarray(mt, np.int32), allv[counts[0]:counts[0] + counts[1]])
    for env, flying, smooth in [({"LSN_DEPTH_SMOOTH": "2,1.5,12", "LSN_FLYING_PIXELS": "1,20"}, (1, 20), SETTING), ({}, None, None)]:
        _, cd, cc, v, t = _want_tick(rig, orc, flying, smooth)
        want = [_H(cd, cc), _H(v, np.asarray(t, np.int32), cd, cc), untouched]
        assert child(CHILD, dict(flow, **env), drop=DROP, timeout=600)[0].split() == want, (flow, env)


@pytest.mark.parametrize("n_ticks,parts", [(1, 1), (8, 2)])
def test_tick_run_equals_the_stages_one_by_one(gpu, orc, n_ticks, parts):
    """lsnTickRun with smoothing on, and with both filters on: the outputs of the stages called one by one on the device (which are the
    restatement's and the oracle's), d_depth_in unchanged; off again: the tick as it was."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion, upload_rigs
    rigs = [_ring(tick=t) for t in range(n_ticks)]
    n = rigs[0].n
    old = os.environ.get("LSN_TICK_PARTS")
    os.environ["LSN_TICK_PARTS"] = str(parts)
    try:
        tp = native.TickPipeline(0, n_ticks, rigs[0].widths, rigs[0].heights)
    finally:
        if old is None:
            del os.environ["LSN_TICK_PARTS"]
        else:
            os.environ["LSN_TICK_PARTS"] = old
    assert tp.parts == parts
    tp.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
    d_in, c_in = upload_rigs(rigs)
    src = b"".join(r.depth_maps.tobytes() for r in rigs)
    d_co, c_co = torch.zeros_like(d_in), torch.zeros_like(c_in)
    verts = torch.zeros((n_ticks, tp.capacity, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((n_ticks, n + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((n_ticks, tp.tri_capacity, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((n_ticks, n + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)

    def run():
        tp.run(d_in.data_ptr(), c_in.data_ptr(), d_co.data_ptr(), c_co.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
        torch.cuda.synchronize()
        return d_co.cpu().numpy(), c_co.cpu().numpy(), verts.cpu().numpy(), off.cpu().numpy(), tri.cpu().numpy(), toff.cpu().numpy()

    plain = run()
    ws, wr = native.depth_smooth_gaussian(*SETTING)
    fus = DeviceFusion.from_rigs(rigs)
    fus.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
    fus.plan.set_depth_smooth(SETTING[0], ws, wr)
    for flying in (None, (1, 20)):
        tp.set_flying_pixels(*(flying or (0, 0)))
        tp.set_depth_smooth(*SETTING)
        with pytest.raises(native.NativeUtilsError):
            tp.set_depth_smooth(4, 1.0, 1.0)                     # refused: the setting stays
        # the stages one by one
        d_f, d_s, d_c, c_c = torch.empty_like(fus.depth), torch.empty_like(fus.depth), torch.empty_like(fus.depth), torch.empty_like(fus.rgb)
        fus.flying_pixels(flying[0] if flying else 0, flying[1] if flying else 0, d_f)
        fus.depth_smooth(d_s, depth=d_f)
        fus.radial_correct_to(d_c, c_c, depth=d_s)
        fus.run_mesh(d_c, c_c)
        torch.cuda.synchronize()
        for _ in range(2):                                        # twice: the second run finds the scratch reserved
            gd, gc, gv, go, gt, gto = run()
            assert d_in.cpu().numpy().tobytes() == src          # d_depth_in stays untouched
            assert gd.tobytes() == d_c.cpu().numpy().tobytes() and gc.tobytes() == c_c.cpu().numpy().tobytes()
            assert np.array_equal(go, fus.offsets.cpu().numpy()) and np.array_equal(gto, fus.tri_offsets.cpu().numpy())
            for k in range(n_ticks):
                assert gv[k, :go[k, -1]].tobytes() == fus.tick_bytes(k).tobytes(), k
                assert np.array_equal(gt[k, :gto[k, -1]], fus.tick_triangles(k)), k
        for k in sorted({0, n_ticks // 2, n_ticks - 1}):         # ... which are the restatement's and the oracle's
            sm, cd, cc, v, t = _want_tick(rigs[k], orc, flying, SETTING)
            assert d_s.cpu().numpy().reshape(n_ticks, -1)[k].view(np.uint8).tobytes() == sm.tobytes(), k
            assert gd.reshape(n_ticks, -1)[k].view(np.uint8).tobytes() == cd.tobytes() and gv[k, :go[k, -1]].tobytes() == v.tobytes(), k
    tp.set_flying_pixels(0, 0)
    tp.set_depth_smooth(0)
    again = run()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain[:2], again[:2])) and np.array_equal(plain[3], again[3])
    od, _ = orc.radial_correction(rigs[0].depth_maps, rigs[0].depth_colors, rigs[0].widths, rigs[0].heights, rigs[0].intr)
    assert plain[0].reshape(n_ticks, -1)[0].view(np.uint8).tobytes() == np.asarray(od).view(np.uint8).tobytes()
    fus.close()
    tp.close()
