#!/usr/bin/env python3
"""Timing of the overlay merge (bgenerate_triangles with the merge switched on) on 8 x 512x424 ring-scene ticks.  Prints one JSON line:

  merge_ms_off / merge_ms_on   generateMeshFromDepthMaps(..., bgenerate_triangles = true) with the merge off / on (C-ABI call + deleteMesh,
                               median wall time of `calls` calls)
  device_ms_per_tick           lsnFusionOverlayMerge on a `ticks`-tick batch already in HBM (HIP events, median of `reps`), per tick
  device_ms_one_tick           the same on a one-tick plan

    python tools/merge_timing.py [calls] [ticks] [reps]
    python tools/merge_timing.py --device-only ...   (only the device-resident part: for rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native  # noqa: E402
from tests import color_cases  # noqa: E402


def _export(rig, merge, calls):
    """The C-ABI call + deleteMesh (what LiveScanServer pays per tick before its own copy), median wall time."""
    import ctypes as C
    L = native.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b = [float(x) for x in rig.bounds]
    prev = native.set_overlay_merge(merge)
    t = []
    try:
        for _ in range(calls + 3):
            m = native.Mesh()
            t0 = time.perf_counter()
            L.generateMeshFromDepthMaps(rig.n, p(rig.depth_maps), p(rig.depth_colors), p(rig.widths), p(rig.heights), p(rig.intr), p(rig.wt),
                                        C.byref(m), False, *b, True)
            L.deleteMesh(C.byref(m))
            t.append((time.perf_counter() - t0) * 1e3)
    finally:
        native.set_overlay_merge(prev)
    return statistics.median(t[3:])


def _device(rigs, reps):
    import torch
    T = len(rigs)
    plan = native.FusionPlan(0, T, rigs[0].widths, rigs[0].heights)
    plan.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
    depth = torch.from_numpy(np.stack([r.depth_maps.view(np.int16) for r in rigs])).cuda()
    rgb = torch.from_numpy(np.stack([r.depth_colors for r in rigs])).cuda()
    N, cap = rigs[0].n, plan.capacity
    verts = torch.zeros((T, cap, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((T, N + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((T, 2 * cap, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((T, N + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)
    plan.run_mesh(depth.data_ptr(), rgb.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
    out = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.overlay_merge(depth.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out[2:]) / T


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls, ticks, reps = (int(args[i]) if len(args) > i else d for i, d in enumerate((20, 16, 10)))
    native.require_gpu()
    rig = color_cases.ring(8)
    res = {"rig": "8 x 512x424 ring scene", "ticks": ticks}
    if "--device-only" not in sys.argv:
        res["merge_ms_off"] = round(_export(rig, False, calls), 4)
        res["merge_ms_on"] = round(_export(rig, True, calls), 4)
    rigs = [color_cases.ring(8, tick=k) for k in range(ticks)]
    for r in rigs[1:]:
        r.intr, r.wt, r.bounds = rigs[0].intr, rigs[0].wt, rigs[0].bounds
    res["device_ms_per_tick"] = round(_device(rigs, reps), 4)
    res["device_ms_one_tick"] = round(_device(rigs[:1], reps), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
