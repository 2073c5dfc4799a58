#!/usr/bin/env python3
"""Timing of depth smoothing (depth_smooth.hip).  Three modes, one JSON line each:

  --kernel   lsnFusionDepthSmooth alone on batches in HBM at r = 1, 2, 3 with the Gaussian tables (1, 1.0, 10), (2, 1.5, 12), (3, 2.0, 15)
             (HIP events, median of `reps`): 64 scene ticks x 8 x 512x424 and 8 ticks x 16 x 1024x1024 (also per tick).  Beside each:
             flying_kernel<R, true> at the same r on the same frames (the sibling stencil with the same traffic) and the 4 B-per-pixel
             copy bound (the device-to-device copy the stage makes when it is off), with the ratios.
  --flows    lsnTickRun on 64 scene ticks x 8 x 512x424 (ticks/s, median of `reps` timed runs of `calls` calls), one
             lsnCorrectAndGenerateMesh and one depthMapAndColorSetRadialCorrection host call on 8 x 512x424 (ms, median of `host_calls`
             calls), with the switch off and -- when the loaded library has it -- at (2, 1.5, 12).
  --ab LIB   "switch off costs nothing": runs `--flows --off-only` in fresh child processes, alternating between this tree's library and
             LIB (the parent commit's libNativeUtils.so, through $LSN_NATIVE_LIB), `pairs` times each, and reports both medians, the
             parent's own run-to-run spread (max - min) and whether the difference of the medians lies within it.

    python tools/depth_smooth_timing.py --kernel [reps]
    python tools/depth_smooth_timing.py --flows [reps] [calls] [host_calls]
    python tools/depth_smooth_timing.py --ab path/to/parent/libNativeUtils.so [pairs]

The 64-tick batches are 8 distinct scene ticks repeated 8 times (the timing does not care, the ray casting on the CPU does)."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402

SETTINGS = {1: (1, 1.0, 10.0), 2: (2, 1.5, 12.0), 3: (3, 2.0, 15.0)}
FLOW_SETTING = SETTINGS[2]


def _scene_rigs(n_ticks, n, w, h, distinct=8):
    return [synth.make_rig("scene", n, w, h, seed=1, tick=t) for t in range(min(distinct, n_ticks))]


def kernel(reps):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    res = {"mode": "kernel", "reps": reps}
    for name, (T, n, w, h) in {"64x8x512x424": (64, 8, 512, 424), "8x16x1024x1024": (8, 16, 1024, 1024)}.items():
        with DeviceFusion.from_rigs(_scene_rigs(T, n, w, h, distinct=8 if w == 512 else 2), T) as fus:
            d_out = torch.empty_like(fus.depth)
            nbytes = 4.0 * fus.depth.numel()
            res[f"{name}_MB"] = round(nbytes / 1e6, 1)
            fus.plan.set_depth_smooth(0)
            copy_ms = timing.event_ms(lambda: fus.depth_smooth(d_out), reps, 2)      # off: the 4 B-per-pixel copy
            res[f"{name}_copy_ms"] = round(copy_ms, 4)
            res[f"{name}_copy_GBps"] = round(nbytes / copy_ms / 1e6, 1)
            for r, setting in SETTINGS.items():
                ws, wr = native.depth_smooth_gaussian(*setting)
                fus.plan.set_depth_smooth(r, ws, wr)
                ms = timing.event_ms(lambda: fus.depth_smooth(d_out), reps, 2)
                fly = timing.event_ms(lambda: fus.flying_pixels(r, 20, d_out), reps, 2)
                res[f"{name}_r{r}_ms"] = round(ms, 4)
                res[f"{name}_r{r}_ms_per_tick"] = round(ms / T, 5)
                res[f"{name}_r{r}_n_range"] = int(wr.size)
                res[f"{name}_r{r}_GBps"] = round(nbytes / ms / 1e6, 1)
                res[f"{name}_r{r}_flying_ms"] = round(fly, 4)
                res[f"{name}_r{r}_over_flying"] = round(ms / fly, 2)
                res[f"{name}_r{r}_over_copy"] = round(ms / copy_ms, 2)
            fus.depth_smooth(d_out)
            res[f"{name}_changed_tick0_r3"] = int(fus.plan.depth_smooth_diagnostics(0)[2])
    print(json.dumps(res))


def flows(reps, calls, host_calls, off_only):
    import torch
    from livescan3d_amd.fusion import upload_rigs
    L = native.lib()
    has = hasattr(L, "lsnSetDepthSmooth")
    res = {"mode": "flows", "library": os.environ.get("LSN_NATIVE_LIB", "in-tree"), "has_smoothing": has, "reps": reps, "calls": calls}
    T, n, w, h = 64, 8, 512, 424
    rigs = _scene_rigs(T, n, w, h)
    rig = rigs[0]
    tp = native.TickPipeline(0, T, rig.widths, rig.heights)
    tp.set_params(rig.intr, rig.wt, rig.bounds)
    d_in, c_in = upload_rigs(rigs, T)
    d_co, c_co = torch.empty_like(d_in), torch.empty_like(c_in)
    verts = torch.zeros((T, tp.capacity, 16), dtype=torch.uint8, device="cuda")
    off = torch.zeros((T, n + 1), dtype=torch.int32, device="cuda")
    tri = torch.zeros((T, tp.tri_capacity, 3), dtype=torch.int32, device="cuda")
    toff = torch.zeros((T, n + 1), dtype=torch.int32, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)

    def tick_rate():
        rates = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                tp.run(d_in.data_ptr(), c_in.data_ptr(), d_co.data_ptr(), c_co.data_ptr(), verts.data_ptr(), off.data_ptr(), tri.data_ptr(), toff.data_ptr(), st)
            torch.cuda.synchronize()
            rates.append(T * calls / (time.perf_counter() - t0))
        return rates[1:]

    def mesh_ms():
        b = [float(x) for x in rig.bounds]
        t = timing.export_call_ms(lambda m, dm, dc: L.lsnCorrectAndGenerateMesh(*timing.rig_pointers(rig, dm, dc)[0], m, *b, 1), host_calls, 3,
                                  frames=lambda: (rig.depth_maps.copy(), rig.depth_colors.copy()))   # the call corrects them in place
        assert native.last_error() == ""
        return t

    def radial_ms():
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        t = []
        for _ in range(host_calls + 3):
            dm, dc = rig.depth_maps.copy(), rig.depth_colors.copy()
            t0 = time.perf_counter()
            L.depthMapAndColorSetRadialCorrection(rig.n, p(dm), p(dc), p(rig.widths), p(rig.heights), p(rig.intr))
            t.append((time.perf_counter() - t0) * 1e3)
        assert native.last_error() == ""
        return t[3:]

    for label, setting in [("off", None)] + ([("on_2_1.5_12", FLOW_SETTING)] if has and not off_only else []):
        if setting:
            tp.set_depth_smooth(*setting)
            prev = native.set_depth_smooth(*setting)
        r = tick_rate()
        res[f"tick_run_ticks_per_s_{label}"] = round(statistics.median(r), 1)
        res[f"tick_run_ticks_per_s_{label}_min_max"] = [round(min(r), 1), round(max(r), 1)]
        res[f"tick_run_vertices_tick0_{label}"] = int(off[0, -1].item())
        for key, fn in (("mesh_call_ms", mesh_ms), ("radial_call_ms", radial_ms)):
            hm = fn()
            res[f"{key}_{label}"] = round(statistics.median(hm), 4)
            res[f"{key}_{label}_min_max"] = [round(min(hm), 4), round(max(hm), 4)]
        if setting:
            native.set_depth_smooth(*prev)
    tp.close()
    print(json.dumps(res))


def ab(parent_lib, pairs):
    runs = {"this": [], "parent": []}
    for i in range(pairs):
        for who in ("parent", "this") if i % 2 else ("this", "parent"):
            env = {k: v for k, v in os.environ.items() if k not in ("LSN_NATIVE_LIB", "LSN_DEPTH_SMOOTH", "LSN_FLYING_PIXELS")}
            if who == "parent":
                env["LSN_NATIVE_LIB"] = os.path.abspath(parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--flows", "--off-only", "5", "20", "30"], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child ({who}) failed with {r.returncode}: {r.stderr[-1500:]}")
            runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"mode": "ab", "pairs": pairs, "parent_has_smoothing": runs["parent"][0]["has_smoothing"], "this_has_smoothing": runs["this"][0]["has_smoothing"]}
    for key in ("tick_run_ticks_per_s_off", "mesh_call_ms_off", "radial_call_ms_off"):
        a, b = [x[key] for x in runs["this"]], [x[key] for x in runs["parent"]]
        spread = max(b) - min(b)
        diff = statistics.median(a) - statistics.median(b)
        res[key] = {"this": a, "parent": b, "median_this": statistics.median(a), "median_parent": statistics.median(b),
                    "difference_of_medians": round(diff, 4), "parent_spread": round(spread, 4), "within_parent_spread": abs(diff) <= spread}
    print(json.dumps(res))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--ab" in sys.argv:
        return ab(args[0], int(args[1]) if len(args) > 1 else 5)
    native.require_gpu()
    if "--kernel" in sys.argv:
        return kernel(int(args[0]) if args else 10)
    reps, calls, host_calls = (int(args[i]) if len(args) > i else d for i, d in enumerate((5, 20, 30)))
    return flows(reps, calls, host_calls, "--off-only" in sys.argv)


if __name__ == "__main__":
    main()
