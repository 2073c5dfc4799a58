#!/usr/bin/env python3
"""Timing of the temporal depth filter (temporal.hip).  One JSON line per mode:

  --kernel   lsnFusionTemporal alone at (64, 20, 2) on batches of scene ticks in HBM, 8 x 512x424 at 1 tick and at 64 ticks, out of place
             (HIP events; `warmup` runs dropped, then min / median / max of `reps`): ms per call, the algorithmic bytes (4 B per pixel
             and tick + 8 B per pixel and call) and the fraction of 8 TB/s they reach.  The history is reset in front of every run, so
             that every run walks the same branches.
  --smooth   the r = 1 depth-smoothing pass (Gaussian tables of (1, 1.0, 10)) on the same two batches with the loaded library: the only
             other per-pixel depth pass, for comparison.
  --compare LIB   --kernel here, then --smooth in a fresh child process on LIB (the parent commit's libNativeUtils.so, through
             $LSN_NATIVE_LIB) and on this tree's library, in the same session; prints all three lines and the ratios.

    python tools/temporal_timing.py --kernel [reps] [warmup]
    python tools/temporal_timing.py --smooth [reps] [warmup]
    python tools/temporal_timing.py --compare path/to/parent/libNativeUtils.so [reps] [warmup]

The 64-tick batch is 8 distinct scene ticks repeated 8 times with a seeded 2 % of the samples dropped per tick (the timing does not care,
the ray casting on the CPU does).  The 1-tick call moves 21 MB, which the 256 MB Infinity Cache holds from run to run: its figure is a
launch-bound call on cached data, not an HBM rate."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from livescan3d_amd import native, synth  # noqa: E402

SETTING = (64, 20, 2)
SMOOTH = (1, 1.0, 10.0)
PEAK_BPS = 8e12
BATCHES = {"1x8x512x424": 1, "64x8x512x424": 64}


def _batch(T):
    import numpy as np
    from livescan3d_amd.fusion import DeviceFusion
    rigs = [synth.make_rig("scene", 8, 512, 424, seed=1, tick=t) for t in range(min(8, T))]
    rng = np.random.default_rng(1)
    for r in rigs:
        dm = r.depth_maps.view("<u2")
        dm[rng.random(dm.size) < 0.02] = 0
    return DeviceFusion.from_rigs(rigs, T)


def _spread(fn, reps, warmup, before=None):
    """(min, median, max) ms of `reps` runs of fn() between two HIP events after `warmup` dropped runs; before(): untimed, ahead of each."""
    import torch
    ms = []
    for _ in range(reps + warmup):
        if before is not None:
            before()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = ms[warmup:]
    return [round(min(ms), 4), round(statistics.median(ms), 4), round(max(ms), 4)]


def kernel(reps, warmup):
    import torch
    res = {"mode": "kernel", "setting": SETTING, "reps": reps, "warmup": warmup}
    for name, T in BATCHES.items():
        with _batch(T) as fus:
            d_out = torch.empty_like(fus.depth)
            fus.set_temporal(*SETTING)
            px = fus.plan.capacity
            nbytes = 4.0 * px * T + 8.0 * px
            ms = _spread(lambda: fus.temporal(d_out), reps, warmup, before=fus.temporal_reset)
            d = sum(fus.temporal_diagnostics(T - 1).sum(axis=0).tolist()) if T > 1 else 0
            res[name] = {"ms_min_median_max": ms, "algorithmic_MB": round(nbytes / 1e6, 1), "GBps_at_median": round(nbytes / ms[1] / 1e6, 1),
                         "fraction_of_8TBps": round(nbytes / (ms[1] * 1e-3) / PEAK_BPS, 4), "last_tick_pixels_with_history": int(d)}
    print(json.dumps(res))
    return res


def smooth(reps, warmup):
    import torch
    res = {"mode": "smooth", "setting": SMOOTH, "reps": reps, "warmup": warmup, "library": os.path.relpath(native.LIB_PATH, ROOT)}
    ws, wr = native.depth_smooth_gaussian(*SMOOTH)
    for name, T in BATCHES.items():
        with _batch(T) as fus:
            d_out = torch.empty_like(fus.depth)
            fus.plan.set_depth_smooth(SMOOTH[0], ws, wr)
            res[name] = {"ms_min_median_max": _spread(lambda: fus.depth_smooth(d_out), reps, warmup)}
    print(json.dumps(res))
    return res


def compare(lib, reps, warmup):
    mine = kernel(reps, warmup)
    lines = {}
    for who, env in (("parent", {"LSN_NATIVE_LIB": os.path.abspath(lib)}), ("this", {})):
        e = {k: v for k, v in os.environ.items() if k != "LSN_NATIVE_LIB"}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--smooth", str(reps), str(warmup)], cwd=ROOT, env=e, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        lines[who] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(lines[who]))
    out = {"mode": "compare"}
    for name in BATCHES:
        t, s = mine[name]["ms_min_median_max"], lines["parent"][name]["ms_min_median_max"]
        out[name] = {"temporal_ms": t[1], "parent_smooth_r1_ms": s[1], "temporal_over_smooth": round(t[1] / s[1], 3),
                     "temporal_spread_ms": round(t[2] - t[0], 4), "smooth_spread_ms": round(s[2] - s[0], 4)}
    print(json.dumps(out))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    native.require_gpu()
    if "--compare" in sys.argv:
        return compare(args[0], int(args[1]) if len(args) > 1 else 30, int(args[2]) if len(args) > 2 else 5)
    reps, warmup = (int(args[i]) if len(args) > i else d for i, d in enumerate((30, 5)))
    return smooth(reps, warmup) if "--smooth" in sys.argv else kernel(reps, warmup)


if __name__ == "__main__":
    main()
