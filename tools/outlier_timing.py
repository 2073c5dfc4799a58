#!/usr/bin/env python3
"""Timing of the outlier filter on 8 x 512x424 scene ticks, at (k, maxDist) = (10, 0.1) and (10, 0.01).  Prints one JSON line:

  merge_ms_off / merge_ms_<k>_<d>      generateMeshFromDepthMaps (flags false, false) with the filter off / on (C-ABI call + deleteMesh, median
                                       wall time of `calls` calls)
  device_ms_per_tick_<T>_<k>_<d>       lsnFusionOutlierFilter on a T-tick batch already in HBM (HIP events, median of `reps`), per tick, for
                                       T = 1 and `ticks`; fusion_mesh_ms_per_tick_<T>: lsnFusionRunMesh on the same batch, for scale
  removed_fraction_<k>_<d>, exact_fraction_<k>_<d>   of the first tick's vertices: removed, decided by the grid pass

    python tools/outlier_timing.py [calls] [ticks] [reps]
    python tools/outlier_timing.py --device-only ...   (only the device-resident part: for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402

SETTINGS = [(10, 0.1), (10, 0.01)]


def _merge(rig, setting, calls):
    L = native.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    b = [float(x) for x in rig.bounds]
    prev = native.set_outlier_filter(*setting)
    t = []
    try:
        for _ in range(calls + 3):
            m = native.Mesh()
            t0 = time.perf_counter()
            L.generateMeshFromDepthMaps(rig.n, p(rig.depth_maps), p(rig.depth_colors), p(rig.widths), p(rig.heights), p(rig.intr), p(rig.wt),
                                        C.byref(m), False, *b, False)
            L.deleteMesh(C.byref(m))
            t.append((time.perf_counter() - t0) * 1e3)
    finally:
        native.set_outlier_filter(*prev)
    assert native.last_error() == ""
    return statistics.median(t[3:])


def _device(rigs, reps, res):
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
    out = torch.empty_like(depth)
    st = int(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        ms = []
        for _ in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms[2:]) / T

    res[f"fusion_mesh_ms_per_tick_{T}"] = round(timed(lambda: plan.run_mesh(depth.data_ptr(), rgb.data_ptr(), verts.data_ptr(), off.data_ptr(),
                                                                             tri.data_ptr(), toff.data_ptr(), st)), 4)
    plan.run(depth.data_ptr(), rgb.data_ptr(), verts.data_ptr(), off.data_ptr(), st)
    torch.cuda.synchronize()
    nv = int(off[0, -1].item())
    for k, d in SETTINGS:
        res[f"device_ms_per_tick_{T}_{k}_{d}"] = round(timed(lambda: plan.outlier_filter(k, d, depth.data_ptr(), verts.data_ptr(), off.data_ptr(),
                                                                                          out.data_ptr(), st)), 4)
        if T == 1:
            dg = plan.outlier_diagnostics(0, nv)
            res[f"removed_fraction_{k}_{d}"] = round(dg["total"] / max(nv, 1), 5)
            res[f"exact_fraction_{k}_{d}"] = round(int(dg["exact_per_sensor"].sum()) / max(nv, 1), 5)
    plan.close()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls, ticks, reps = (int(args[i]) if len(args) > i else d for i, d in enumerate((20, 16, 10)))
    native.require_gpu()
    rig = synth.make_rig("scene", 8, 512, 424, seed=1)
    res = {"rig": "8 x 512x424 scene", "ticks": ticks}
    if "--device-only" not in sys.argv:
        res["merge_ms_off"] = round(_merge(rig, (0, 0.0), calls), 4)
        for k, d in SETTINGS:
            res[f"merge_ms_{k}_{d}"] = round(_merge(rig, (k, d), calls), 4)
    rigs = [synth.make_rig("scene", 8, 512, 424, seed=1, tick=t) for t in range(ticks)]
    _device(rigs[:1], reps, res)
    _device(rigs, reps, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
