"""Background subtraction inside the flows that start at raw frames: lsnTickRun after lsnTickSetBackground / lsnTickBackgroundLearn, and the
host exports (depthMapAndColorSetRadialCorrection, lsnCorrectAndGenerateMesh) with lsnSetBackground / $LSN_BACKGROUND / lsnLearnBackground
in the one-device flow, with a group per sensor, and sharded over the one GPU listed three times; with the temporal filter in front and
the flying-pixel filter behind.

Bar: byte for byte.  The tick equals the device stages chained one by one (temporal -> background -> flying -> smooth -> correct -> mesh),
whose second stage equals the restatement (tests/background_ref.py); the exports equal a simulation of the lane's rule (a model per rig and
generation, learning calls that pass through) on the restatements, then the existing oracle.  Wherever frames are compared, the
restatement's own counts must first show foreground, background and removed blobs, so that no comparison is vacuous.  With the switch off
the exports' bytes are the pinned ones: the existing pins hold that."""
import hashlib
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import background_ref as ref, color_cases, flying_ref, temporal_ref
from tests.support import child

pytestmark = pytest.mark.gpu

SETTING = (20, 4, 12)
TEMPORAL = (64, 20, 2)
FLYING = (1, 20)
SMOOTH = (1, 1.0, 10.0)
OF = 8


def frames(n_ticks, size, n=3, empty=(), seed=5):
    """n_ticks frames of an n-sensor ring (the scene's own +-2 mm jitter from tick to tick) with a fifth of the samples dropped; the ticks
    of `empty` show the room without its subjects."""
    rng = np.random.default_rng(seed)
    rigs = [color_cases.ring(n, sizes=[size] * n, of=OF, tick=t) for t in range(n_ticks)]
    for t, r in enumerate(rigs):
        dm = r.depth_maps.view("<u2")
        if t in empty:
            dm[:] = np.concatenate([synth.scene_frame(1, t, s, OF, *size, subjects=False)[0].ravel() for s in range(n)])
        dm[rng.random(dm.size) < 0.2] = 0
    return rigs


@pytest.mark.parametrize("stages", ["background", "temporal+background+flying+smooth"])
@pytest.mark.parametrize("parts", [1, 2])
def test_tick_run_equals_the_stages_one_by_one(gpu, parts, stages):
    import torch
    from livescan3d_amd.fusion import DeviceFusion, upload_rigs
    n_ticks = 8
    size = (40, 24)
    rigs = frames(n_ticks, size, n=2)
    room = frames(n_ticks, size, n=2, empty=range(n_ticks), seed=6)
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
    d_room, _ = upload_rigs(room)
    src = b"".join(r.depth_maps.tobytes() for r in rigs)
    maps = np.frombuffer(src, "<u2").reshape(n_ticks, -1)
    room_maps = np.frombuffer(b"".join(r.depth_maps.tobytes() for r in room), "<u2").reshape(n_ticks, -1)
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
    full = stages != "background"
    fus = DeviceFusion.from_rigs(rigs)
    fus.set_background(*SETTING)
    tp.set_background(*SETTING)
    with pytest.raises(native.NativeUtilsError):
        tp.set_background(5000, 0, 0)                               # refused: the setting stays
    if full:
        ws, wr = native.depth_smooth_gaussian(*SMOOTH)
        fus.plan.set_depth_smooth(SMOOTH[0], ws, wr)
        fus.set_temporal(*TEMPORAL)
        tp.set_temporal(*TEMPORAL)
        tp.set_flying_pixels(*FLYING)
        tp.set_depth_smooth(*SMOOTH)
    d_t, d_b, d_f, d_s, d_c = (torch.empty_like(fus.depth) for _ in range(5))
    c_c = torch.empty_like(fus.rgb)

    def chain_learn():
        last = d_room
        if full:
            fus.temporal(d_t, depth=last)
            last = d_t
        fus.background_learn(depth=last)

    def chain():
        """The stages one by one on the 8-tick plan, whose history and model continue from call to call like the tick object's."""
        last = fus.depth
        if full:
            fus.temporal(d_t)
            last = d_t
        fus.background(d_b, depth=last)
        last = d_b
        if full:
            fus.flying_pixels(*FLYING, d_f, depth=d_b)
            fus.depth_smooth(d_s, depth=d_f)
            last = d_s
        fus.radial_correct_to(d_c, c_c, depth=last)
        fus.run_mesh(d_c, c_c)
        torch.cuda.synchronize()
        o, to = fus.offsets.cpu().numpy(), fus.tri_offsets.cpu().numpy()
        return (d_c.cpu().numpy().tobytes(), c_c.cpu().numpy().tobytes(), o.tobytes(), to.tobytes(),
                b"".join(fus.tick_bytes(k).tobytes() for k in range(n_ticks)), b"".join(fus.tick_triangles(k).tobytes() for k in range(n_ticks)))

    widths, heights = list(rigs[0].widths), list(rigs[0].heights)
    # nothing learned: every sample is unknown; the blob pass alone works
    want0 = chain()
    got0 = run()
    assert got0 == want0
    # learn the empty room (through the temporal filter when that is on), then subtract
    chain_learn()
    tp.background_learn(d_room.data_ptr(), st)
    torch.cuda.synchronize()
    assert d_room.cpu().numpy().tobytes() == b"".join(r.depth_maps.tobytes() for r in room)        # a learning pass writes no maps
    model = fus.background_model()
    if not full:
        assert np.array_equal(model, ref.learn(np.zeros(maps.shape[1], np.uint16), room_maps))
    want1 = chain()
    seen = d_t.cpu().numpy().view("<u2").reshape(n_ticks, -1) if full else maps
    w_b, counts, _ = ref.run(seen, model, widths, heights, *SETTING)
    assert d_b.cpu().numpy().view("<u2").reshape(n_ticks, -1).tobytes() == w_b.tobytes()
    tot = counts.sum(axis=(0, 1))
    assert tot[ref.FOREGROUND] > 200 and tot[ref.BACKGROUND] > 200 and tot[ref.COMPONENTS_REMOVED] > 0 and tot[ref.COMPONENTS] > tot[ref.COMPONENTS_REMOVED], tot
    assert [fus.background_diagnostics(t).tolist() for t in range(n_ticks)] == counts.tolist()
    got1 = run()
    assert got1 == want1 and got1[0] != plain[0] and got1[0] != got0[0]
    # a reset: nothing learned again
    tp.background_reset(st)
    fus.background_reset()
    if full:
        tp.temporal_reset(st)
        fus.temporal_reset()
        assert run() == chain() == want0                            # (the histories restart together, where the first run started)
    else:
        assert run() == want0
    # off again: the tick as it was
    tp.set_background(0)
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
from tests.test_background_flows_gpu import frames, SIZE
H = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()
E0, E1, S2, S3 = frames(4, SIZE, empty=(0, 1))
A = lambda r: (r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr)
px = SIZE[0] * SIZE[1]
out = []
def radial(r, n=None):
    a = A(r) if n is None else (r.depth_maps[:2 * px * n], r.depth_colors[:3 * px * n], r.widths[:n], r.heights[:n], r.intr[:7 * n])
    gd, gc = native.radial_correction(*a)
    return H(np.asarray(gd).view(np.uint8), gc)
out += [radial(E0), radial(E1), radial(S2), radial(S3)]              # two learning calls pass through, then subtraction
native.learn_background(1)                                            # a generation bump clears the model: one learning call
out += [radial(E1), radial(S2)]
radial(E0, n=1)                                                       # a changed rig ...
out += [radial(E0), radial(S2)]                                       # ... and the first one again: cleared, learning re-armed
r = S3
v, t, d, c = native.correct_and_generate_mesh(*A(r), r.wt, r.bounds)  # the other export that starts at raw frames, same model
out.append(H(v, np.asarray(t, np.int32), np.asarray(d).view(np.uint8), c))
uv, ut = native.generate_mesh_from_depth_maps(*A(r), r.wt, r.bounds)
out.append(H(uv, np.asarray(ut, np.int32)))                           # the merge export never runs the stage
prev = native.set_background(0)
out.append(radial(S2) + str(prev))                                    # the switch off: today's bytes
print(" ".join(out).replace(", ", ","))
"""

SIZE = (96, 80)
DROP = ("LSN_BACKGROUND", "LSN_TEMPORAL_FILTER", "LSN_DEPTH_SMOOTH", "LSN_FLYING_PIXELS", "LSN_OUTLIER_FILTER", "LSN_HOST_PATH", "LSN_HOST_GROUP",
        "LSN_HOST_DEVICES")


def _H(*a):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()


class Lane:
    """The rule of include/NativeUtils.h for the exports, on the restatements: one temporal history and one model per rig; a changed rig or
    generation zeroes the model and arms `learn_calls` learning calls, which pass their maps through."""

    def __init__(self, orc, temporal, flying, learn_calls):
        self.orc, self.temporal, self.flying, self.learn_calls = orc, temporal, flying, learn_calls
        self.rig, self.state, self.model, self.left = None, None, None, 0
        self.counts = []

    def learn(self, n_calls):
        self.learn_calls, self.model, self.left = n_calls, None, n_calls

    def call(self, r, on=True):
        """-> (corrected depth as uint8, corrected colours) of one call of the whole rig r."""
        dm = r.depth_maps
        rig = (list(r.widths), list(r.heights))
        if rig != self.rig:
            self.rig, self.state, self.model, self.left = rig, None, None, self.learn_calls
        if self.temporal:
            dm, self.state = temporal_ref.run_packed(dm, self.state, *TEMPORAL)
        if on:
            if self.model is None:
                self.model = np.zeros(dm.size // 2, np.uint16)
            if self.left > 0:
                self.left -= 1
                self.model = ref.learn_packed(self.model, dm)
            else:
                dm, counts = ref.run_packed(dm, self.model, r.widths, r.heights, *SETTING)
                self.counts.append(counts.sum(axis=0))
        if self.flying:
            dm, _ = flying_ref.filter_packed(dm, r.widths, r.heights, *FLYING)
        cd, cc = self.orc.radial_correction(dm, r.depth_colors, r.widths, r.heights, r.intr)
        return np.asarray(cd).view(np.uint8).ravel(), np.asarray(cc).ravel()


class One:
    """The first sensor of a rig as a rig of its own."""

    def __init__(self, r):
        px = SIZE[0] * SIZE[1]
        self.depth_maps, self.depth_colors, self.widths, self.heights, self.intr = r.depth_maps[:2 * px], r.depth_colors[:3 * px], r.widths[:1], r.heights[:1], r.intr[:7]


FLOWS = {
    "default": {},
    "group1": {"LSN_HOST_GROUP": "1"},
    "shard3": {"LSN_HOST_DEVICES": "0,0,0"},
    "default-temporal": {"LSN_TEMPORAL_FILTER": "64,20,2"},
    "default-flying": {"LSN_FLYING_PIXELS": "1,20"},
    "shard3-temporal-flying": {"LSN_HOST_DEVICES": "0,0,0", "LSN_TEMPORAL_FILTER": "64,20,2", "LSN_FLYING_PIXELS": "1,20"},
}


@pytest.mark.parametrize("flow", list(FLOWS))
def test_host_exports_learn_then_subtract(gpu, orc, flow):
    """$LSN_BACKGROUND=margin,rel_q,min_pixels,2 in a child process per flow: two pass-through calls, subtraction, a generation bump, a rig
    change, the other export, the merge export, the switch off -- against the simulated lane."""
    env = FLOWS[flow]
    E0, E1, S2, S3 = frames(4, SIZE, empty=(0, 1))
    lane = Lane(orc, "LSN_TEMPORAL_FILTER" in env, "LSN_FLYING_PIXELS" in env, 2)
    off_lane = Lane(orc, "LSN_TEMPORAL_FILTER" in env, "LSN_FLYING_PIXELS" in env, 0)
    want = [_H(*lane.call(r)) for r in (E0, E1, S2, S3)]
    off = [_H(*off_lane.call(r, on=False)) for r in (E0, E1, S2, S3)]
    assert want[:2] == off[:2] and want[2] != off[2] and want[3] != off[3]         # learning calls pass through; subtraction does not
    tot = np.sum(lane.counts, axis=0)
    assert tot[ref.FOREGROUND] > 1000 and tot[ref.BACKGROUND] > 1000 and tot[ref.UNKNOWN] > 0 and tot[ref.COMPONENTS_REMOVED] > 0, tot
    lane.learn(1)
    want += [_H(*lane.call(E1)), _H(*lane.call(S2))]
    if not lane.temporal:
        assert want[5] != want[2]                                   # the model of E1 alone is not the model of E0 and E1
    lane.call(One(E0))
    want += [_H(*lane.call(E0)), _H(*lane.call(S2))]
    cd, cc = lane.call(S3)
    r = S3
    v, _, t = orc.generate_mesh(cd, cc, r.widths, r.heights, r.intr, r.wt, r.bounds)
    want.append(_H(v, np.asarray(t, np.int32), cd, cc))
    mv, _, mt = orc.generate_mesh(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr, r.wt, r.bounds)
    want.append(_H(mv, np.asarray(mt, np.int32)))
    want.append(_H(*lane.call(S2, on=False)) + "(%d,%d,%d)" % SETTING)
    got = child(CHILD, dict(env, LSN_BACKGROUND="%d,%d,%d,2" % SETTING), drop=DROP, timeout=600)[0].split()
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b]


def test_environment_switch_refuses_what_the_setter_refuses(gpu):
    """A malformed or out-of-range $LSN_BACKGROUND leaves the stage off, with a message on stderr; lsnSetBackground refuses the same values
    and keeps its setting; lsnLearnBackground refuses a negative count."""
    code = "from livescan3d_amd import native; print(native.set_background(0))"
    for text in ("20,4,12,", "20,256,12,2"):
        line, err = child(code, {"LSN_BACKGROUND": text}, drop=DROP)
        assert line == "(0, 0, 0)" and "LSN_BACKGROUND" in err, (text, line, err)
    # (a well-formed value is what test_host_exports_learn_then_subtract runs on: its child reads the triple back)
    assert native.set_background(30, 8, 1) == (0, 0, 0)
    for bad in [(4096, 8, 1), (30, 256, 1), (30, 8, -1)]:
        with pytest.raises(native.NativeUtilsError, match="lsnSetBackground"):
            native.set_background(*bad)
    with pytest.raises(native.NativeUtilsError, match="lsnLearnBackground"):
        native.learn_background(-1)
    native.learn_background(0)
    assert native.set_background(0) == (30, 8, 1)
