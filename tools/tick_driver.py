#!/usr/bin/env python3
"""Dev helper: the chained tick (radial correction out of place -> vertices -> triangulation) on T ticks x 8 sensors, for kernel traces.
usage: python3 tools/tick_driver.py [scene|noise] [ticks] [reps]"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from livescan3d_amd import synth
from livescan3d_amd.fusion import DeviceFusion, upload_rigs

kind = sys.argv[1] if len(sys.argv) > 1 else "scene"
T = int(sys.argv[2]) if len(sys.argv) > 2 else 64
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
S, w, h = 8, 512, 424
dev = torch.device("cuda", 0)
rig0 = synth.make_rig("scene", S, w, h, seed=4, tick=0, bounds=synth.CROP_BOUNDS)
if kind == "noise":
    depth, rgb = synth.noise_frames_torch(dev, 1, T, S, w, h)
    depth, rgb = depth.view(T, -1), rgb.view(T, -1)
else:
    rigs = [synth.make_rig("scene", S, w, h, seed=4, tick=k) for k in range(min(T, 8))]
    depth, rgb = upload_rigs(rigs, T, 0)
fus = DeviceFusion(T, rig0.widths, rig0.heights, device=0)
fus.set_params(rig0.intr, rig0.wt, rig0.bounds)
d2, c2 = torch.empty_like(depth), torch.empty_like(rgb)
for rep in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fus.radial_correct_to(d2, c2, depth, rgb)
    fus.run_mesh(d2, c2)
    torch.cuda.synchronize()
    print(kind, T, "ticks:", round(1e3 * (time.perf_counter() - t0), 3), "ms", flush=True)
print("vertices/tick", float(fus.offsets[:, -1].float().mean()), "triangles/tick", float(fus.tri_offsets[:, -1].float().mean()))
