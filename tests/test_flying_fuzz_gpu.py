"""Seeded random rigs through the flying-pixel filter's flows, in the style of tests/test_fuzz_gpu.py: frames from 1 x 1 up, 1-8 sensors of
different sizes (widths on both sides of every multiple of 8, so both the 16-byte and the element-wise forms of the kernel run, and
tiles that end inside a frame), r = 1-4 (the on-chip forms and the plain one), random thresholds (the corners -1, 0, 65535 among them),
lenses that fold the frame.  The radial export, the tick as one call and lsnTickRun must return what tests/flying_ref.py followed by the
oracle returns, bit for bit; d_depth_out of the device call and the outputs of lsnTickRun sit between guard bands that must stay
intact (tests/test_bounds_gpu.py)."""
import os

import numpy as np
import pytest

from livescan3d_amd import native, synth
from tests import flying_ref
from tests.support import Guarded

pytestmark = pytest.mark.gpu

SCALE = max(1, int(os.environ.get("LSN_FUZZ_SCALE", "1")))
N_CASES = 60 * SCALE


def _random_rig(rng):
    n = int(rng.integers(1, 9))
    depths, rgbs, intr, wt = [], [], [], []
    for s in range(n):
        shape = int(rng.integers(0, 5))
        if shape == 0:
            w, h = int(rng.integers(1, 12)), int(rng.integers(1, 12))          # around and below the windows
        elif shape == 1:
            w, h = 8 * int(rng.integers(1, 40)) + int(rng.integers(-1, 2)), int(rng.integers(3, 40))   # either side of a multiple of 8
        elif shape == 2:
            w, h = 8 * int(rng.integers(2, 40)), int(rng.integers(4, 60))      # the 16-byte form, tiles that end inside the frame
        elif shape == 3:
            w, h = int(rng.integers(200, 700)), int(rng.integers(1, 10))       # long and flat
        else:
            w, h = int(rng.integers(16, 300)), int(rng.integers(16, 100))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            d, c = synth.noise_frame(int(rng.integers(1, 1000)), 0, s, w, h)
        elif kind == 1 and w >= 32 and h >= 24:
            d, c = synth.scene_frame(int(rng.integers(1, 100)), 0, s, n, w, h)
        elif kind == 2:                                                        # a smooth surface with steps, stripes and dots of holes
            yy, xx = np.mgrid[0:h, 0:w]
            d = (1200 + 3 * xx + 2 * yy + rng.integers(0, 30, size=(h, w)) + 400 * ((xx // 17 + yy // 11) % 2)).astype(np.uint16)
            d[:, :: int(rng.integers(2, 9))] = 0
            d[rng.random((h, w)) < 0.05] = 0
            c = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        else:                                                                  # the whole u16 range, half of it holes
            d = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
            d[rng.random((h, w)) < 0.5] = 0
            c = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        depths.append(np.ascontiguousarray(d)); rgbs.append(np.ascontiguousarray(c))
        k = synth.kinect_intrinsics(w, h).copy()
        k[4:7] = rng.uniform(-0.3, 0.3, size=3).astype(np.float32)
        if rng.random() < 0.15:                                                # a lens that folds the frame onto itself
            k[4:7] = rng.uniform(-4.0, 4.0, size=3).astype(np.float32)
        intr.append(k.astype(np.float32))
        wt.append(synth.pack_pose(*synth.ring_pose(s, n)))
    r = int(rng.integers(1, 5))
    thr = int(rng.choice([-1, 0, 1, 5, 20, 50, 300, 4000, 65534, 65535, int(rng.integers(0, 70000))]))
    return synth.Rig(depths, rgbs, np.concatenate(intr), np.concatenate(wt), np.array([-6, -6, -6, 6, 6, 6], np.float32)), r, thr


@pytest.mark.parametrize("seed", range(N_CASES))
def test_random_rig_through_every_entry(gpu, orc, seed):
    import torch
    from livescan3d_amd.fusion import upload_rig
    rng = np.random.default_rng(7000 + seed)
    rig, r, thr = _random_rig(rng)
    what = f"seed {seed}: sizes {list(zip(rig.widths.tolist(), rig.heights.tolist()))} r {r} thr {thr}"
    fm, removed = flying_ref.filter_packed(rig.depth_maps, rig.widths, rig.heights, r, thr)
    cd, cc = orc.radial_correction(fm, rig.depth_colors, rig.widths, rig.heights, rig.intr)
    cd, cc = np.asarray(cd).view(np.uint8).ravel(), np.asarray(cc).ravel()
    want_v, _, want_t = orc.generate_mesh(cd, cc, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    dev = torch.device("cuda", 0)
    npix = int(np.sum(rig.widths.astype(np.int64) * rig.heights))

    # the device call between guard bands, from an input at an odd 2-byte offset half of the time (the element-wise form)
    plan = native.FusionPlan(0, 1, rig.widths, rig.heights)
    shift = 2 * int(rng.integers(0, 2))
    src = Guarded(torch, 2 * npix + shift, dev)
    src.body()[shift:].copy_(torch.from_numpy(rig.depth_maps.copy()))
    dst = Guarded(torch, 2 * npix, dev)
    plan.flying_pixels(r, thr, src.ptr + shift, dst.ptr)
    per, total = plan.flying_diagnostics(0)
    assert dst.body().cpu().numpy().tobytes() == fm.tobytes(), what + " [device call]"
    assert dst.intact() and src.intact(), what + " [device call: guard bands]"
    assert per.tolist() == removed.tolist() and total == int(removed.sum()), what + " [diagnostics]"
    plan.close()

    # the radial export and the tick as one call
    gd, gc = native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, flying_pixels=(r, thr))
    assert np.asarray(gd).view(np.uint8).tobytes() == cd.tobytes() and np.asarray(gc).tobytes() == cc.tobytes(), what + " [radial export]"
    v, t, d3, c3 = native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds,
                                                    flying_pixels=(r, thr))
    assert v.tobytes() == want_v.tobytes() and np.array_equal(np.asarray(t).reshape(-1, 3), want_t), what + " [tick as one call]"
    assert np.asarray(d3).view(np.uint8).tobytes() == cd.tobytes() and np.asarray(c3).tobytes() == cc.tobytes(), what + " [maps of the one call]"

    # lsnTickRun on two copies of the tick, every output between guard bands
    T = 2
    tp = native.TickPipeline(0, T, rig.widths, rig.heights)
    tp.set_params(rig.intr, rig.wt, rig.bounds)
    tp.set_flying_pixels(r, thr)
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
