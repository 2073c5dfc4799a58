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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native  # noqa: E402
from tests import color_cases  # noqa: E402
from tools import timing  # noqa: E402


def _merge(rig, merge, calls):
    """The C-ABI call + deleteMesh (what LiveScanServer pays per tick before its own copy), median wall time."""
    L = native.lib()
    frames, b = timing.rig_pointers(rig)
    prev = native.set_overlay_merge(merge)
    try:
        return statistics.median(timing.export_call_ms(lambda m: L.generateMeshFromDepthMaps(*frames, m, False, *b, True), calls, 3))
    finally:
        native.set_overlay_merge(prev)


def _device(rigs, reps):
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run_mesh()
        return timing.event_ms(fus.overlay_merge, reps, 2) / len(rigs)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls, ticks, reps = (int(args[i]) if len(args) > i else d for i, d in enumerate((20, 16, 10)))
    native.require_gpu()
    rig = color_cases.ring(8)
    res = {"rig": "8 x 512x424 ring scene", "ticks": ticks}
    if "--device-only" not in sys.argv:
        res["merge_ms_off"] = round(_merge(rig, False, calls), 4)
        res["merge_ms_on"] = round(_merge(rig, True, calls), 4)
    rigs = [color_cases.ring(8, tick=k) for k in range(ticks)]
    res["device_ms_per_tick"] = round(_device(rigs, reps), 4)
    res["device_ms_one_tick"] = round(_device(rigs[:1], reps), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
