"""Seeded rigs of the ring-rig fuzzer (tests/support.py) through depth smoothing: 1-4 sensors, every sensor its own size from 1 x 1 up or
one size for all (widths on both sides of the multiples of 8, so both forms of the kernel run), random r.  The device call runs with
random valid tables (zeros in both, n_range anywhere in 1..1024), lsnTickRun with the Gaussian tables of random sigmas -- and, half of
the time, with the flying-pixel filter in front.  Both must return what tests/depth_smooth_ref.py (behind tests/flying_ref.py, in front
of the oracle) returns, bit for bit, with every output between guard bands that stay intact."""
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import depth_smooth_cases as cases, depth_smooth_ref as ref, flying_ref
from tests.support import Guarded, ragged_or_equal, ring_rig

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("LSN_FUZZ_SCALE", "1")))
N_CASES = 32 * SCALE
SIZES = ragged_or_equal(150, 40, [8, 64, 96, 129, 136], [1, 5, 17, 33])


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_rig_through_the_device_call_and_the_tick(gpu, orc, seed):
    import torch
    from livescan3d_amd.fusion import upload_rig
    rng = np.random.default_rng(9100 + seed)
    rig = ring_rig(rng, 4, [4, 8], SIZES)
    r = int(rng.integers(1, 4))
    ws, wr = cases.random_tables(rng, r)
    # a few millimetres of noise on the valid pixels, so that the range weights matter
    dm = rig.depth_maps.view("<u2").astype(np.int64)
    dm = np.where(dm != 0, np.clip(dm + rng.integers(-5, 6, size=dm.size), 1, 65535), 0).astype("<u2")
    rig.depth_maps = dm.view(np.uint8)
    what = f"seed {seed}: sizes {list(zip(rig.widths.tolist(), rig.heights.tolist()))} r {r} n_range {wr.size}"
    dev = torch.device("cuda", 0)
    npix = int(np.sum(rig.widths.astype(np.int64) * rig.heights))

    # the device call between guard bands, from an input at an odd 2-byte offset half of the time (the element-wise form)
    plan = native.FusionPlan(0, 1, rig.widths, rig.heights)
    plan.set_depth_smooth(r, ws, wr)
    shift = 2 * int(rng.integers(0, 2))
    src = Guarded(torch, 2 * npix + shift, dev)
    src.body()[shift:].copy_(torch.from_numpy(rig.depth_maps.copy()))
    dst = Guarded(torch, 2 * npix, dev)
    plan.depth_smooth(src.ptr + shift, dst.ptr)
    ch, mv, total = plan.depth_smooth_diagnostics(0)
    want, changed, moved = ref.smooth_packed(rig.depth_maps, rig.widths, rig.heights, r, ws, wr)
    assert dst.body().cpu().numpy().tobytes() == want.tobytes(), what + " [device call]"
    assert dst.intact() and src.intact(), what + " [device call: guard bands]"
    assert ch.tolist() == changed.tolist() and mv.tolist() == moved.tolist() and total == int(changed.sum()), what + " [diagnostics]"
    plan.close()

    # lsnTickRun on two copies of the tick, every output between guard bands
    sigma_s, sigma_r = float(rng.uniform(0.4, 3.0)), float(rng.uniform(1.0, 40.0))
    flying = (int(rng.integers(1, 4)), int(rng.choice([5, 20, 300]))) if rng.random() < 0.5 else None
    gws, gwr = native.depth_smooth_gaussian(r, sigma_s, sigma_r)
    fm = flying_ref.filter_packed(rig.depth_maps, rig.widths, rig.heights, *flying)[0] if flying else rig.depth_maps
    sm, _, _ = ref.smooth_packed(fm, rig.widths, rig.heights, r, gws, gwr)
    cd, cc = orc.radial_correction(sm, rig.depth_colors, rig.widths, rig.heights, rig.intr)
    cd, cc = np.asarray(cd).view(np.uint8).ravel(), np.asarray(cc).ravel()
    want_v, _, want_t = orc.generate_mesh(cd, cc, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    what += f" sigmas {sigma_s:.3f} {sigma_r:.3f} flying {flying}"
    T = 2
    tp = native.TickPipeline(0, T, rig.widths, rig.heights)
    tp.set_params(rig.intr, rig.wt, rig.bounds)
    tp.set_depth_smooth(r, sigma_s, sigma_r)
    if flying:
        tp.set_flying_pixels(*flying)
    d_in, c_in = upload_rig(rig, T, 0)
    n = rig.n
    outs = {"depth": Guarded(torch, T * 2 * npix, dev), "colors": Guarded(torch, T * 3 * npix, dev), "verts": Guarded(torch, T * 16 * tp.capacity, dev),
            "off": Guarded(torch, T * 4 * (n + 1), dev), "tri": Guarded(torch, T * 12 * tp.tri_capacity, dev), "toff": Guarded(torch, T * 4 * (n + 1), dev)}
    tp.run(d_in.data_ptr(), c_in.data_ptr(), outs["depth"].ptr, outs["colors"].ptr, outs["verts"].ptr, outs["off"].ptr, outs["tri"].ptr, outs["toff"].ptr)
    torch.cuda.synchronize()
    assert all(g.intact() for g in outs.values()), what + " [lsnTickRun: guard bands]"
    assert d_in.cpu().numpy()[0].tobytes() == rig.depth_maps.tobytes(), what + " [lsnTickRun: input untouched]"
    off = outs["off"].body().cpu().numpy().view(np.int32).reshape(T, n + 1)
    toff = outs["toff"].body().cpu().numpy().view(np.int32).reshape(T, n + 1)
    gd = outs["depth"].body().cpu().numpy().reshape(T, -1)
    gc = outs["colors"].body().cpu().numpy().reshape(T, -1)
    gv = outs["verts"].body().cpu().numpy().reshape(T, -1)
    gt = outs["tri"].body().cpu().numpy().view(np.int32).reshape(T, -1, 3)
    for k in range(T):
        assert gd[k].tobytes() == cd.tobytes() and gc[k].tobytes() == cc.tobytes(), what + f" [lsnTickRun maps, tick {k}]"
        assert off[k, -1] == len(want_v) and gv[k, :16 * off[k, -1]].tobytes() == want_v.tobytes(), what + f" [lsnTickRun vertices, tick {k}]"
        assert np.array_equal(gt[k, :toff[k, -1]], want_t), what + f" [lsnTickRun triangles, tick {k}]"
    tp.close()
