#!/usr/bin/env python3
"""Timing of the colour transfer (bcolor_transfer) on 8 x 512x424 ring-scene ticks.  Prints one JSON line:

  merge_ms_plain / merge_ms_color   generateMeshFromDepthMaps with the flag false / true (C-ABI call + deleteMesh, median wall time of `calls` calls)
  device_ms_per_tick                lsnFusionColorTransfer on a `ticks`-tick batch already in HBM (HIP events, median of `reps`), per tick
  device_ms_one_tick                the same on a one-tick plan

    python tools/color_timing.py [calls] [ticks] [reps]
    python tools/color_timing.py --device-only ...   (only the device-resident part: for rocprofv3 --kernel-trace --stats)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native  # noqa: E402
from tests import color_cases  # noqa: E402
from tools import timing  # noqa: E402


def _merge(rig, color, calls):
    """The C-ABI call + deleteMesh (what LiveScanServer pays per tick before its own copy), median wall time."""
    L = native.lib()
    frames, b = timing.rig_pointers(rig)
    t = timing.export_call_ms(lambda m: L.generateMeshFromDepthMaps(*frames, m, bool(color), *b, False), calls, 3)
    assert native.last_error() == ""
    return statistics.median(t)


def _device(rigs, reps):
    from livescan3d_amd.fusion import DeviceFusion
    with DeviceFusion.from_rigs(rigs) as fus:
        fus.run()
        # colour transfer is in place: each rep starts from the uncorrected cloud (the refill is outside the timed region)
        return timing.event_ms(fus.color_transfer, reps, 2, before=fus.run) / len(rigs)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls, ticks, reps = (int(args[i]) if len(args) > i else d for i, d in enumerate((20, 16, 10)))
    native.require_gpu()
    rig = color_cases.ring(8)
    res = {"rig": "8 x 512x424 ring scene", "ticks": ticks}
    if "--device-only" not in sys.argv:
        res["merge_ms_plain"] = round(_merge(rig, False, calls), 4)
        res["merge_ms_color"] = round(_merge(rig, True, calls), 4)
    rigs = [color_cases.ring(8, tick=k) for k in range(ticks)]
    res["device_ms_per_tick"] = round(_device(rigs, reps), 4)
    res["device_ms_one_tick"] = round(_device(rigs[:1], reps), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
