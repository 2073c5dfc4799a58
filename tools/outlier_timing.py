#!/usr/bin/env python3
"""Timing of the outlier filter on 8 x 512x424 scene ticks, at (k, maxDist) = (10, 0.1) and (10, 0.01).  Prints one JSON line:

  merge_ms_off / merge_ms_<k>_<d>      generateMeshFromDepthMaps (flags false, false) with the filter off / on (C-ABI call + deleteMesh, median
                                       wall time of `calls` calls)
  device_ms_per_tick_<T>_<k>_<d>       lsnFusionOutlierFilter on a T-tick batch already in HBM (HIP events, median of `reps`), per tick, for
                                       T = 1 and `ticks`; fusion_mesh_ms_per_tick_<T>: lsnFusionRunMesh on the same batch, for scale
  removed_fraction_<k>_<d>, exact_fraction_<k>_<d>   of the first tick's vertices: removed, decided by the grid pass

    python tools/outlier_timing.py [calls] [ticks] [reps]
    python tools/outlier_timing.py --device-only ...   (only the device-resident part: for rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402

SETTINGS = [(10, 0.1), (10, 0.01)]


def _merge(rig, setting, calls):
    L = native.lib()
    frames, b = timing.rig_pointers(rig)
    prev = native.set_outlier_filter(*setting)
    try:
        t = timing.export_call_ms(lambda m: L.generateMeshFromDepthMaps(*frames, m, False, *b, False), calls, 3)
    finally:
        native.set_outlier_filter(*prev)
    assert native.last_error() == ""
    return statistics.median(t)


def _device(rigs, reps, res):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    T = len(rigs)
    with DeviceFusion.from_rigs(rigs) as fus:
        out = torch.empty_like(fus.depth)
        res[f"fusion_mesh_ms_per_tick_{T}"] = round(timing.event_ms(fus.run_mesh, reps, 2) / T, 4)
        fus.run()
        nv = int(fus.host_offsets()[0, -1])
        for k, d in SETTINGS:
            res[f"device_ms_per_tick_{T}_{k}_{d}"] = round(timing.event_ms(lambda: fus.outlier_filter(k, d, out), reps, 2) / T, 4)
            if T == 1:
                dg = fus.plan.outlier_diagnostics(0, nv)
                res[f"removed_fraction_{k}_{d}"] = round(dg["total"] / max(nv, 1), 5)
                res[f"exact_fraction_{k}_{d}"] = round(int(dg["exact_per_sensor"].sum()) / max(nv, 1), 5)


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
