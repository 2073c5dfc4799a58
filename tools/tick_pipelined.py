#!/usr/bin/env python3
"""Dev experiment: the chained tick on two plans / two streams (half the ticks each) against one plan on one stream."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from livescan3d_amd import synth
from livescan3d_amd.fusion import DeviceFusion, upload_rigs

kind = sys.argv[1] if len(sys.argv) > 1 else "scene"
T = int(sys.argv[2]) if len(sys.argv) > 2 else 64
parts = int(sys.argv[3]) if len(sys.argv) > 3 else 2
S, w, h = 8, 512, 424
dev = torch.device("cuda", 0)
rig0 = synth.make_rig("scene", S, w, h, seed=4, tick=0, bounds=synth.CROP_BOUNDS)
if kind == "noise":
    depth, rgb = synth.noise_frames_torch(dev, 1, T, S, w, h)
    depth, rgb = depth.view(T, -1), rgb.view(T, -1)
else:
    rigs = [synth.make_rig("scene", S, w, h, seed=4, tick=k) for k in range(min(T, 8))]
    depth, rgb = upload_rigs(rigs, T, 0)

def make(n_ticks):
    fus = DeviceFusion(n_ticks, rig0.widths, rig0.heights, device=0)
    fus.set_params(rig0.intr, rig0.wt, rig0.bounds)
    return fus, torch.empty((n_ticks, depth.shape[1]), dtype=depth.dtype, device=dev), torch.empty((n_ticks, rgb.shape[1]), dtype=rgb.dtype, device=dev)

def tick(p, d, c, st):
    fus, d2, c2 = p
    fus.radial_correct_to(d2, c2, d, c, st)
    fus.run_mesh(d2, c2, st)

def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps

one = make(T)
st0 = torch.cuda.current_stream()
ms1 = timed(lambda: tick(one, depth, rgb, st0))
print(kind, T, "ticks, one plan / one stream:", round(ms1, 3), "ms ->", round(T / ms1, 1), "k ticks/s", flush=True)
del one
torch.cuda.empty_cache()
per = T // parts
ps = [make(per) for _ in range(parts)]
streams = [torch.cuda.Stream() for _ in range(parts)]
def piped():
    for i in range(parts):
        tick(ps[i], depth[i * per:(i + 1) * per], rgb[i * per:(i + 1) * per], streams[i])
ms2 = timed(piped)
print(kind, T, f"ticks, {parts} plans / {parts} streams:", round(ms2, 3), "ms ->", round(T / ms2, 1), "k ticks/s", flush=True)
