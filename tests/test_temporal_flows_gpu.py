"""The temporal depth filter inside the flows that start at raw frames: lsnTickRun after lsnTickSetTemporal, and the host exports
(depthMapAndColorSetRadialCorrection, lsnCorrectAndGenerateMesh) with lsnSetTemporalFilter / $LSN_TEMPORAL_FILTER in the one-device flow,
with a group per sensor, and sharded over the one GPU listed twice.

Bar: byte for byte.  The tick equals the device stages chained one by one (temporal -> flying -> smooth -> correct -> mesh), whose first
stage equals the restatement (tests/temporal_ref.py); the exports equal the restatement, then tests/flying_ref.py, then the existing
oracle.  Wherever frames are compared, the restatement's own branches must first show blends and fills, so that no comparison is vacuous.
With the switch off the exports' bytes are the pinned ones: the existing pins hold that."""
import hashlib
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_cases, depth_smooth_ref, flying_ref, temporal_ref as ref
from tests.support import child

pytestmark = pytest.mark.gpu

SETTING = (64, 20, 2)
FLYING = (1, 20)
SMOOTH = (1, 1.0, 10.0)


def frames(n_ticks, size, seed=5):
    """n_ticks frames of a two-sensor ring (the scene's own +-2 mm jitter from tick to tick) with a fifth of the samples dropped."""
    rng = np.random.default_rng(seed)
    rigs = [color_cases.ring(2, sizes=[size] * 2, of=8, tick=t) for t in range(n_ticks)]
    for r in rigs:
        dm = r.depth_maps.view("<u2")
        dm[rng.random(dm.size) < 0.2] = 0
    return rigs


@pytest.mark.parametrize("stages", ["temporal", "temporal+flying+smooth"])
@pytest.mark.parametrize("parts", [1, 2])
def test_tick_run_equals_the_stages_one_by_one(gpu, parts, stages):
    import torch
    from livescan3d_amd.fusion import DeviceFusion, upload_rigs
    n_ticks = 8
    rigs = frames(n_ticks, (24, 10))
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
    maps = np.frombuffer(src, "<u2").reshape(n_ticks, -1)
    d_co, c_co = torch.zeros_like(d_in), torch.zeros_like(c_in)
    verts = torch.zeros((n_ticks, tp.capacity, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((n_ticks, n + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((n_ticks, tp.tri_capacity, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((n_ticks, n + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)

    def run():
        tp.run(d_in.data_ptr(), c_in.data_ptr(), d_co.data_ptr(), c_co.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
        torch.cuda.synchronize()
        assert d_in.cpu().numpy().tobytes() == src                  # d_depth_in stays untouched
        o, to = off.cpu().numpy(), toff.cpu().numpy()
        v, t = verts.cpu().numpy(), tri.cpu().numpy()
        return (d_co.cpu().numpy().tobytes(), c_co.cpu().numpy().tobytes(), o.tobytes(), to.tobytes(),
                b"".join(v[k, :o[k, -1]].tobytes() for k in range(n_ticks)), b"".join(t[k, :to[k, -1]].tobytes() for k in range(n_ticks)))

    plain = run()
    full = stages != "temporal"
    fus = DeviceFusion.from_rigs(rigs)
    fus.set_temporal(*SETTING)
    tp.set_temporal(*SETTING)
    with pytest.raises(native.NativeUtilsError):
        tp.set_temporal(64, 5000, 0)                                # refused: the setting stays
    if full:
        ws, wr = native.depth_smooth_gaussian(*SMOOTH)
        fus.plan.set_depth_smooth(SMOOTH[0], ws, wr)
        tp.set_flying_pixels(*FLYING)
        tp.set_depth_smooth(*SMOOTH)
    d_t, d_f, d_s, d_c = (torch.empty_like(fus.depth) for _ in range(4))
    c_c = torch.empty_like(fus.rgb)

    def chain():
        """The stages one by one on the 8-tick plan, whose history continues from call to call like the tick object's."""
        fus.temporal(d_t)
        last = d_t
        if full:
            fus.flying_pixels(*FLYING, d_f, depth=d_t)
            fus.depth_smooth(d_s, depth=d_f)
            last = d_s
        fus.radial_correct_to(d_c, c_c, depth=last)
        fus.run_mesh(d_c, c_c)
        torch.cuda.synchronize()
        o, to = fus.offsets.cpu().numpy(), fus.tri_offsets.cpu().numpy()
        return (d_c.cpu().numpy().tobytes(), c_c.cpu().numpy().tobytes(), o.tobytes(), to.tobytes(),
                b"".join(fus.tick_bytes(k).tobytes() for k in range(n_ticks)), b"".join(fus.tick_triangles(k).tobytes() for k in range(n_ticks)))

    # the first run starts from no history, and its first stage is the restatement's
    want1 = chain()
    w_t, w_state, br = ref.run(maps, np.zeros(maps.shape[1], np.uint32), *SETTING)
    assert d_t.cpu().numpy().view("<u2").reshape(n_ticks, -1).tobytes() == w_t.tobytes()
    assert (br == ref.BLEND).sum() > 50 and (br == ref.FILL).sum() > 20 and (br == ref.EXPIRE).sum() > 0     # not vacuous
    assert np.array_equal(fus.temporal_state(), w_state)
    got1 = run()
    assert got1 == want1 and got1[0] != plain[0]
    # a second run continues the first's history
    want2 = chain()
    assert d_t.cpu().numpy().view("<u2").reshape(n_ticks, -1).tobytes() == ref.run(maps, w_state, *SETTING)[0].tobytes()
    got2 = run()
    assert got2 == want2 and got2[0] != got1[0]
    # a reset restarts it
    tp.temporal_reset(st)
    assert run() == want1
    # off again (the history stays where it is): the tick as it was
    tp.set_temporal(0)
    tp.set_flying_pixels(0, 0)
    tp.set_depth_smooth(0)
    assert run() == plain
    fus.close()
    tp.close()


CHILD = r"""
import hashlib, sys
import numpy as np
from livescan3d_amd import native
from tests.test_temporal_flows_gpu import frames
H = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()
rigs = frames(3, (96, 80))
A = lambda r: (r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr)
out = []
def radial(r, n=None):
    a = A(r) if n is None else (r.depth_maps[:2 * 96 * 80 * n], r.depth_colors[:3 * 96 * 80 * n], r.widths[:n], r.heights[:n], r.intr[:7 * n])
    gd, gc = native.radial_correction(*a)
    return H(np.asarray(gd).view(np.uint8), gc)
out += [radial(rigs[0]), radial(rigs[1]), radial(rigs[2])]           # three consecutive calls: one history
radial(rigs[0], n=1)                                                  # a changed rig ...
out.append(radial(rigs[0]))                                           # ... and the first one again: both start fresh
out.append(radial(rigs[1]))                                           # continued
native.reset_temporal_filter()
out.append(radial(rigs[1]))                                           # fresh
r = rigs[2]
v, t, d, c = native.correct_and_generate_mesh(*A(r), r.wt, r.bounds)  # continued, by the other export that starts at raw frames
out.append(H(v, np.asarray(t, np.int32), np.asarray(d).view(np.uint8), c))
ply = native.last_mesh_ply()                                          # lsnLastMesh* serve the filtered call's mesh ...
mv, mt = native.generate_mesh_from_depth_maps(np.asarray(d).view(np.uint8), c, r.widths, r.heights, r.intr, r.wt, r.bounds)
out.append(str(ply == native.last_mesh_ply() and len(ply) > 1000 and mv.tobytes() == v.tobytes()))   # ... which is the mesh of its maps
uv, ut = native.generate_mesh_from_depth_maps(*A(r), r.wt, r.bounds)
out.append(H(uv, np.asarray(ut, np.int32)))                               # the merge export never filters
prev = native.set_temporal_filter(0)
out.append(radial(rigs[0]) + str(prev))                               # the switch off: today's bytes
print(" ".join(out).replace(", ", ","))
"""

DROP = ("LSN_TEMPORAL_FILTER", "LSN_DEPTH_SMOOTH", "LSN_FLYING_PIXELS", "LSN_OUTLIER_FILTER", "LSN_HOST_PATH", "LSN_HOST_GROUP", "LSN_HOST_DEVICES")


def _H(*a):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()


FLOWS = [{}, {"LSN_HOST_GROUP": "1"}, {"LSN_HOST_DEVICES": "0,0"}]


@pytest.mark.parametrize("flow,smooth", [(f, False) for f in FLOWS] + [(f, True) for f in FLOWS],
                         ids=["default", "group1", "shard2", "default-smooth", "group1-smooth", "shard2-smooth"])
def test_host_exports_keep_one_history_per_rig(gpu, orc, flow, smooth):
    """$LSN_TEMPORAL_FILTER with $LSN_FLYING_PIXELS -- and, in the second stage set, $LSN_DEPTH_SMOOTH: all three stages -- in a child
    process per flow: the restatement, tests/flying_ref.py, (tests/depth_smooth_ref.py with the library's own tables,) then the oracle."""
    rigs = frames(3, (96, 80))
    tables = native.depth_smooth_gaussian(*SMOOTH) if smooth else None

    def behind(dm, r, smoothed):
        """The stages behind the temporal filter, then the correction: (corrected depth, corrected colours)."""
        dm, _ = flying_ref.filter_packed(dm, r.widths, r.heights, *FLYING)
        if smoothed:
            dm, changed, _ = depth_smooth_ref.smooth_packed(dm, r.widths, r.heights, SMOOTH[0], *tables)
            assert (changed > 0).all()
        cd, cc = orc.radial_correction(dm, r.depth_colors, r.widths, r.heights, r.intr)
        return np.asarray(cd).view(np.uint8).ravel(), np.asarray(cc).ravel()

    def tick(r, state, smoothed=smooth):
        """One call: (state', corrected depth, corrected colours)."""
        dm, state, = ref.run_packed(r.depth_maps, state, *SETTING)
        return (state,) + behind(dm, r, smoothed)

    def off(r):
        return _H(*behind(r.depth_maps, r, smooth))

    want, s = [], None
    for r in rigs:                                                    # three consecutive calls
        s, cd, cc = tick(r, s)
        want.append(_H(cd, cc))
    # the history did something: tick 2 from the history differs from tick 2 from none, and fills happened
    _, _, br = ref.run(np.stack([r.depth_maps.view("<u2") for r in rigs]), np.zeros(rigs[0].depth_maps.size // 2, np.uint32), *SETTING)
    assert (br == ref.FILL).sum() > 100 and (br == ref.BLEND).sum() > 1000
    assert want[2] != _H(*tick(rigs[2], None)[1:]) and want[1] != off(rigs[1]) and want[0] == off(rigs[0])     # (a first tick is the identity)
    s0, cd, cc = tick(rigs[0], None)
    if smooth:                                                        # smoothing did something: tick 1 differs from the unsmoothed one
        assert want[1] != _H(*tick(rigs[1], s0, smoothed=False)[1:])
    want.append(_H(cd, cc))                                           # fresh after the changed rig
    assert want[3] == want[0]
    s1, cd, cc = tick(rigs[1], s0)
    want.append(_H(cd, cc))                                           # continued
    s1, cd, cc = tick(rigs[1], None)
    want.append(_H(cd, cc))                                           # fresh after the reset
    assert want[5] != want[4]
    r = rigs[2]
    _, cd, cc = tick(r, s1)
    v, _, t = orc.generate_mesh(cd, cc, r.widths, r.heights, r.intr, r.wt, r.bounds)
    want.append(_H(v, np.asarray(t, np.int32), cd, cc))
    want.append("True")
    mv, _, mt = orc.generate_mesh(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr, r.wt, r.bounds)
    want.append(_H(mv, np.asarray(mt, np.int32)))
    want.append(off(rigs[0]) + "(64,20,2)")
    env = dict(flow, LSN_TEMPORAL_FILTER="64,20,2", LSN_FLYING_PIXELS="1,20", **({"LSN_DEPTH_SMOOTH": "1,1.0,10"} if smooth else {}))
    got = child(CHILD, env, drop=DROP, timeout=600)[0].split()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_environment_switch_refuses_what_the_setter_refuses(gpu):
    """A malformed or out-of-range $LSN_TEMPORAL_FILTER leaves the stage off, with a message on stderr; lsnSetTemporalFilter refuses the
    same values and keeps its setting."""
    code = "from livescan3d_amd import native; print(native.set_temporal_filter(0))"
    for text in ("64,20", "64,20,256"):
        line, err = child(code, {"LSN_TEMPORAL_FILTER": text}, drop=DROP)
        assert line == "(0, 0, 0)" and "LSN_TEMPORAL_FILTER" in err, (text, line, err)
    # (a well-formed value is what test_host_exports_keep_one_history_per_rig runs on: its child reads the triple back)
    assert native.set_temporal_filter(128, 30, 1) == (0, 0, 0)
    for bad in [(257, 20, 2), (64, 4096, 2), (64, 20, -1)]:
        with pytest.raises(native.NativeUtilsError, match="lsnSetTemporalFilter"):
            native.set_temporal_filter(*bad)
    assert native.set_temporal_filter(0) == (128, 30, 1)
