#!/usr/bin/env python3
"""Timing of background subtraction (background.hip) on 64 ticks x 8 x 512x424 in HBM.  One JSON line:

  learn            lsnFusionBackgroundLearn on 64 ticks of the empty room (the model reset in front of every run)
  classify_only    lsnFusionBackground at (20, 4, 0), out of place, on the scene ticks against the learned empty room
  classify_blobs   the same at (20, 4, 64): classification, then the blob pass (16 ticks at a time)
  temporal         lsnFusionTemporal at (64, 20, 2) on the same scene batch in the same run (the history reset in front of every run)
  copy             a device-to-device copy of the batch's maps (2 B in + 2 B out per pixel and tick): the box's copy rate

    python tools/background_timing.py [reps] [warmup]

HIP events; `warmup` runs dropped, then min / median / max ms of `reps`, the algorithmic bytes of the pointwise passes and their rate.  The
scene batch is 8 distinct ticks of synth.scene_frame repeated 8 times, the room the same ticks without the subjects; the share of the
scene's samples the stage removes is a figure of this synthetic scene, not of real Kinect frames."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from livescan3d_amd import native, synth  # noqa: E402
from temporal_timing import _spread  # noqa: E402

T, N, W, H = 64, 8, 512, 424
CLASSIFY, BLOBS, TEMPORAL = (20, 4, 0), (20, 4, 64), (64, 20, 2)


def main():
    import numpy as np
    import torch
    from livescan3d_amd.fusion import DeviceFusion, upload_rigs
    args = sys.argv[1:]
    reps, warmup = (int(args[i]) if len(args) > i else d for i, d in enumerate((30, 5)))
    native.require_gpu()
    rigs = [synth.make_rig("scene", N, W, H, seed=1, tick=t) for t in range(8)]
    room = [synth.make_rig("scene", N, W, H, seed=1, tick=t) for t in range(8)]
    for t, r in enumerate(room):
        r.depth_maps.view("<u2")[:] = np.concatenate([synth.scene_frame(1, t, s, N, W, H, subjects=False)[0].ravel() for s in range(N)])
    res = {"batch": f"{T}x{N}x{W}x{H}", "reps": reps, "warmup": warmup}
    with DeviceFusion.from_rigs(rigs, T) as fus:
        d_room, _ = upload_rigs(room, T)
        d_out = torch.empty_like(fus.depth)
        px = fus.plan.capacity
        point = 4.0 * px * T                                        # 2 B in + 2 B out per pixel and tick

        def line(ms, nbytes):
            return {"ms_min_median_max": ms, "algorithmic_MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / ms[1] / 1e6, 1)}

        res["copy"] = line(_spread(lambda: d_out.copy_(fus.depth), reps, warmup), point)
        res["learn"] = line(_spread(lambda: fus.background_learn(depth=d_room), reps, warmup, before=fus.background_reset), 2.0 * px * T + 4.0 * px)
        fus.background_reset()
        fus.background_learn(depth=d_room)
        fus.set_background(*CLASSIFY)
        res["classify_only"] = line(_spread(lambda: fus.background(d_out), reps, warmup), point)   # (the 3.5 MB model stays in the caches)
        c0 = np.sum([fus.background_diagnostics(t).sum(axis=0) for t in range(8)], axis=0)
        fus.set_background(*BLOBS)
        res["classify_blobs"] = line(_spread(lambda: fus.background(d_out), reps, warmup), point)
        c1 = np.sum([fus.background_diagnostics(t).sum(axis=0) for t in range(8)], axis=0)
        fus.set_temporal(*TEMPORAL)
        res["temporal"] = line(_spread(lambda: fus.temporal(d_out), reps, warmup, before=fus.temporal_reset), point + 8.0 * px)
        res["blobs_alone_ms"] = round(res["classify_blobs"]["ms_min_median_max"][1] - res["classify_only"]["ms_min_median_max"][1], 4)
        res["over_temporal"] = {k: round(res[k]["ms_min_median_max"][1] / res["temporal"]["ms_min_median_max"][1], 3)
                                for k in ("learn", "classify_only", "classify_blobs")}
        res["over_copy"] = {k: round(res[k]["ms_min_median_max"][1] / res["copy"]["ms_min_median_max"][1], 3)
                            for k in ("learn", "classify_only", "classify_blobs")}
        names = ("foreground", "unknown", "background", "components", "components_removed", "pixels_removed")
        res["synthetic_scene_counts_8_ticks"] = {"classify_only": dict(zip(names, map(int, c0))), "classify_blobs": dict(zip(names, map(int, c1)))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
