"""Stream hand-over of the two stages that carry state from call to call (lsn::StageState: the temporal filter's history, background
subtraction's model): a reset queued on one stream, then the next call on another.  Every operation that touches the state records its
stream, so the call waits for the reset.  On a plan and on a tick object.

Bar: byte for byte against the numpy restatements started from no history / nothing learned.  These are guards, not proofs: the order is
deterministic with the record, and a build without it usually wins the race all the same."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import background_ref, color_cases, temporal_ref

pytestmark = pytest.mark.gpu

SIZES = [(136, 40), (128, 16)]      # a tile edge in x and in y, one width that is no multiple of 128
N_TICKS = 2
TEMPORAL = (64, 20, 2)
BACKGROUND = (20, 4, 0)             # no blob pass: the counts are the classification's alone


def rigs():
    rng = np.random.default_rng(11)
    out = [color_cases.ring(len(SIZES), sizes=SIZES, of=8, tick=t) for t in range(N_TICKS)]
    for r in out:
        dm = r.depth_maps.view("<u2")
        dm[rng.random(dm.size) < 0.2] = 0
    return out


@pytest.fixture
def second_stream(gpu):
    s = native.lib().lsnStreamCreate(0)
    assert s
    yield s
    assert native.lib().lsnStreamDestroy(0, s) == 0


def test_plan_filters_behind_a_reset_on_another_stream(gpu, second_stream):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rr = rigs()
    maps = np.stack([r.depth_maps.view("<u2") for r in rr])
    with DeviceFusion.from_rigs(rr) as fus:
        fus.set_temporal(*TEMPORAL)
        # a valid history that changes every outcome: every pixel 40 mm in front of tick 0's sample, or at 1 m where that has none
        old = temporal_ref.pack(np.where(maps[0] != 0, (maps[0].astype(np.int64) + 40) * 256, 1000 * 256), 1)
        assert temporal_ref.state_ok(old)
        fus.set_temporal_state(old)
        want_out, want_state, _ = temporal_ref.run(maps, np.zeros(maps.shape[1], np.uint32), *TEMPORAL)
        stale_out, _, _ = temporal_ref.run(maps, old, *TEMPORAL)
        assert stale_out.tobytes() != want_out.tobytes()            # (not vacuous: the old history would show)
        fus.plan.temporal_reset(second_stream)
        out = torch.empty_like(fus.depth)
        fus.temporal(out)
        torch.cuda.synchronize()
        assert out.cpu().numpy().view("<u2").reshape(N_TICKS, -1).tobytes() == want_out.tobytes()
        assert fus.temporal_state().tobytes() == want_state.tobytes()


def test_tick_runs_behind_resets_on_another_stream(gpu, second_stream):
    import torch
    from livescan3d_amd.fusion import DeviceFusion, upload_rigs
    rr = rigs()
    n = rr[0].n
    maps = np.stack([r.depth_maps.view("<u2") for r in rr])
    widths, heights = list(rr[0].widths), list(rr[0].heights)
    tp = native.TickPipeline(0, N_TICKS, rr[0].widths, rr[0].heights)
    tp.set_params(rr[0].intr, rr[0].wt, rr[0].bounds)
    d_in, c_in = upload_rigs(rr)
    d_co, c_co = torch.zeros_like(d_in), torch.zeros_like(c_in)
    verts = torch.zeros((N_TICKS, tp.capacity, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((N_TICKS, n + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((N_TICKS, tp.tri_capacity, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((N_TICKS, n + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)

    def run():
        tp.run(d_in.data_ptr(), c_in.data_ptr(), d_co.data_ptr(), c_co.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
        torch.cuda.synchronize()
        o = off.cpu().numpy()
        return d_co.cpu().numpy().tobytes(), o.tobytes(), b"".join(verts[k, :o[k, -1]].cpu().numpy().tobytes() for k in range(N_TICKS))

    # the temporal filter: a first run starts from no history, a second continues it, a third behind a reset on the other stream starts over
    tp.set_temporal(*TEMPORAL)
    first = run()
    assert run() != first                                           # (not vacuous: the history shows)
    tp.temporal_reset(second_stream)
    assert run() == first
    tp.set_temporal(0)

    # background subtraction: learn the batch itself, reset on the other stream, run -- the next run's counts must show every sample
    # unknown.  The same stages one by one on a plan read the counts (the tick object has no diagnostics export of its own): its model
    # is reset on the run's own stream, so it states what "nothing learned" gives.
    tp.set_background(*BACKGROUND)
    nothing = run()
    tp.background_learn(d_in.data_ptr(), st)
    learned = run()
    assert learned != nothing                                       # (not vacuous: the model shows)
    tp.background_learn(d_in.data_ptr(), st)
    tp.background_reset(second_stream)
    assert run() == nothing
    with DeviceFusion.from_rigs(rr) as fus:
        fus.set_background(*BACKGROUND)
        d_b, d_c, c_c = torch.empty_like(fus.depth), torch.empty_like(fus.depth), torch.empty_like(fus.rgb)
        fus.background_learn()
        fus.background_reset()
        fus.background(d_b)
        fus.radial_correct_to(d_c, c_c, depth=d_b)
        torch.cuda.synchronize()
        assert d_c.cpu().numpy().tobytes() == nothing[0]
        _, counts, _ = background_ref.run(maps, np.zeros(maps.shape[1], np.uint16), widths, heights, *BACKGROUND)
        got = [fus.background_diagnostics(t).tolist() for t in range(N_TICKS)]
        assert got == counts.tolist()
        assert all(c[background_ref.FOREGROUND] == 0 and c[background_ref.BACKGROUND] == 0 and c[background_ref.UNKNOWN] > 0
                   for per_tick in got for c in per_tick), got
    tp.close()
