#!/usr/bin/env python3
"""Dev helper: one pass of radial correction + full mesh on 16 ticks x 8 sensors (scene data), for kernel traces."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from livescan3d_amd import synth
from livescan3d_amd.fusion import DeviceFusion

T, S, w, h = 16, 8, 512, 424
kind = os.environ.get("DRV_KIND", "scene")
rigs = [synth.make_rig(kind, S, w, h, seed=1, tick=k, bounds=synth.CROP_BOUNDS) for k in range(2)]
fus = DeviceFusion.from_rigs(rigs, T)
for rep in range(2):
    d2, c2 = fus.depth.clone(), fus.rgb.clone()
    fus.radial_correct(d2, c2)
    fus.run_mesh(d2, c2)
    torch.cuda.synchronize()
print("vertices/tick", float(fus.offsets[:, -1].float().mean()), "triangles/tick", float(fus.tri_offsets[:, -1].float().mean()))
