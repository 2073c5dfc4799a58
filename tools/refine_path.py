#!/usr/bin/env python3
"""LiveScanServer's "Refine calibration" through the library, two ways, on one rig of scene frames (default 8 x 512x424, 2 x 10 iterations):

  --baseline  the path through the reference's exports: depthMapAndColorSetRadialCorrection (in place, on the same two arrays refilled
              with the raw frames before every repeat; the refill is not timed) + n x generateVerticesFromDepthMap (with the copy out of the Mesh, what
              KinectServer.CopyMeshToVerticesWithColoursArray does) + the X, Y, Z strip on the host + lsnRefine.  Works with any build of
              the library, so with $LSN_NATIVE_LIB it times the parent commit's.
  --onecall   lsnRefineFromDepthMaps(correct_radial = 1): once the way LiveScanServer would call it (no clouds back) and once with the
              refined clouds returned.
  --ab LIB    fresh child processes, alternating: --baseline on LIB (the parent commit's libNativeUtils.so) and --onecall on this tree's
              library, `pairs` times each; reports both medians, each side's run-to-run spread (max - min of the children's medians), the
              baseline's parts, and whether the refined clouds have the same digest on both sides.

  --plane     both refine passes on the SAME resident tick (DeviceFusion: run_mesh -> normals): lsnRefineVertices (point-to-point) and
              lsnRefineVerticesPlane (point-to-plane), alternating; ms per call and per ICP iteration (a call is refine_iters x S ICP
              runs of icp_iters iterations, with its copies and the one synchronise), each with its spread, and how far each pass moved
              the clouds.

    python tools/refine_path.py --baseline [repeats] [S w h] [refine_iters icp_iters]
    python tools/refine_path.py --plane [repeats] [S w h] [refine_iters icp_iters]
    python tools/refine_path.py --onecall [repeats] [S w h] [refine_iters icp_iters]
    python tools/refine_path.py --ab path/to/parent/libNativeUtils.so [pairs] [repeats]

Every call is complete on return (its results are host arrays), so the times are wall clock around the calls; one warm-up pass first.
One JSON line per mode."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from livescan3d_amd import native, synth  # noqa: E402


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _rig(S, w, h):
    return synth.make_rig("scene", S, w, h, seed=4, perturb=True)


def _world(rig):
    wt = rig.wt.reshape(-1, 12)
    return wt[:, 3:].copy().reshape(-1), wt[:, :3].copy().reshape(-1)


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def baseline(repeats, S, w, h, iters):
    L = native.lib()
    rig = _rig(S, w, h)
    b = [float(x) for x in rig.bounds]
    parts = {k: [] for k in ("radial", "vertices", "strip", "refine", "total")}
    digest = None
    dm, dc = rig.depth_maps.copy(), rig.depth_colors.copy()     # long-lived arrays, as a host keeps them: refilled, not reallocated
    for rep in range(repeats + 1):
        np.copyto(dm, rig.depth_maps)
        np.copyto(dc, rig.depth_colors)
        wR, wt = _world(rig)
        Rs, Ts = np.zeros(9 * S, np.float32), np.zeros(3 * S, np.float32)
        t0 = time.perf_counter()
        L.depthMapAndColorSetRadialCorrection(S, _p(dm), _p(dc), _p(rig.widths), _p(rig.heights), _p(rig.intr))
        t1 = time.perf_counter()
        blocks = []
        for i in range(S):
            mesh = native.Mesh()
            L.generateVerticesFromDepthMap(_p(dm), _p(dc), _p(rig.widths), _p(rig.heights), _p(rig.intr), _p(rig.wt), C.byref(mesh), *b, i)
            blocks.append(np.frombuffer(C.string_at(mesh.vertices, mesh.nVertices * 16), dtype=native.VERTEX_DTYPE))
            L.deleteMesh(C.byref(mesh))
        t2 = time.perf_counter()
        clouds = [np.stack([v["X"], v["Y"], v["Z"]], axis=1) for v in blocks]      # MainWindowForm.cs:318-327
        t3 = time.perf_counter()
        counts = np.array([len(c) for c in clouds], np.int32)
        ptrs = (C.c_void_p * S)(*[c.ctypes.data for c in clouds])
        rc = L.lsnRefine(0, S, C.cast(ptrs, C.c_void_p), _p(counts), iters[0], iters[1], _p(wR), _p(wt), _p(Rs), _p(Ts))
        t4 = time.perf_counter()
        assert rc == 0 and native.last_error() == "", native.last_error()
        if rep == 0:
            digest = synth.digest(np.concatenate(clouds))
            continue
        assert synth.digest(np.concatenate(clouds)) == digest
        for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            parts[k].append(1e3 * dt)
    res = {"mode": "baseline", "library": os.environ.get("LSN_NATIVE_LIB", "in-tree"), "rig": [S, w, h], "iters": list(iters), "repeats": repeats,
           "points": int(counts.sum()), "digest": digest, "poses_digest": synth.digest(np.concatenate([Rs, Ts, wR, wt]))}
    res.update({k: _stats(v) for k, v in parts.items()})
    print(json.dumps(res))


def onecall(repeats, S, w, h, iters):
    L = native.lib()
    rig = _rig(S, w, h)
    b = [float(x) for x in rig.bounds]
    clouds = np.zeros(int(np.sum(rig.widths.astype(np.int64) * rig.heights)) * 3, np.float32)
    counts = np.zeros(S, np.int32)
    wt_out, Rs, Ts = np.zeros(12 * S, np.float32), np.zeros(9 * S, np.float32), np.zeros(3 * S, np.float32)
    times = {"lean": [], "with_clouds": []}
    for rep in range(repeats + 1):
        for key, (c_ptr, n_ptr) in (("lean", (None, None)), ("with_clouds", (_p(clouds), _p(counts)))):
            t0 = time.perf_counter()
            rc = L.lsnRefineFromDepthMaps(S, _p(rig.depth_maps), _p(rig.depth_colors), _p(rig.widths), _p(rig.heights), _p(rig.intr), _p(rig.wt),
                                          *b, 1, iters[0], iters[1], _p(wt_out), None, None, _p(Rs), _p(Ts), c_ptr, n_ptr)
            dt = time.perf_counter() - t0
            assert rc == 0, native.last_error()
            if rep > 0:
                times[key].append(1e3 * dt)
    wt12 = wt_out.reshape(-1, 12)
    res = {"mode": "onecall", "rig": [S, w, h], "iters": list(iters), "repeats": repeats, "points": int(counts.sum()),
           "digest": synth.digest(clouds[:3 * int(counts.sum())]),
           "poses_digest": synth.digest(np.concatenate([Rs, Ts, wt12[:, 3:].reshape(-1), wt12[:, :3].reshape(-1)])),
           "kept_bytes": native.refine_release(0)}
    res.update({k: _stats(v) for k, v in times.items()})
    print(json.dumps(res))


def plane(repeats, S, w, h, iters):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rig = _rig(S, w, h)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        normals = fus.normals()
        torch.cuda.synchronize()
        total = int(fus.host_offsets()[0, -1])
        before = fus.vertices[0, :total].view(torch.float32)[:, 1:4].cpu().numpy()
        out = torch.zeros((total, 3), dtype=torch.float32, device=fus.device)
        passes = {"point_to_point": lambda: fus.refine(0, *iters, clouds_out=out),
                  "point_to_plane": lambda: fus.refine_plane(0, normals, *iters, clouds_out=out)}
        times, moved, digests = {k: [] for k in passes}, {}, {}
        for rep in range(repeats + 1):
            for key, call in passes.items():
                t0 = time.perf_counter()
                call()
                dt = time.perf_counter() - t0
                if rep == 0:
                    after = out.cpu().numpy()
                    moved[key], digests[key] = float(np.abs(after - before).max()), synth.digest(after)
                else:
                    times[key].append(1e3 * dt)
        res = {"mode": "plane", "rig": [S, w, h], "iters": list(iters), "repeats": repeats, "points": total,
               "zero_normals": fus.plan.normals_diagnostics(0)["zero_normals"]}
        n_iterations = iters[0] * S * iters[1]
        for key in passes:
            st = _stats(times[key])
            res[key] = dict(st, per_iteration_ms=round(st["median_ms"] / n_iterations, 5), moved_max_m=round(moved[key], 6), digest=digests[key])
        res["kept_bytes"] = native.refine_release(0)
    print(json.dumps(res))


def ab(parent_lib, pairs, repeats):
    runs = {"baseline": [], "onecall": []}
    for i in range(pairs):
        for mode in ("onecall", "baseline") if i % 2 else ("baseline", "onecall"):
            env = {k: v for k, v in os.environ.items() if k != "LSN_NATIVE_LIB"}
            if mode == "baseline":
                env["LSN_NATIVE_LIB"] = os.path.abspath(parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--" + mode, str(repeats)], env=env, cwd=ROOT, capture_output=True,
                               text=True, timeout=900)
            if r.returncode != 0:
                sys.exit(f"child ({mode}) failed with {r.returncode}: {r.stderr[-1500:]}")
            runs[mode].append(json.loads(r.stdout.strip().splitlines()[-1]))

    def side(rows, key):
        m = [x[key]["median_ms"] for x in rows]
        return {"medians_ms": m, "median_ms": round(statistics.median(m), 4), "spread_ms": round(max(m) - min(m), 4)}

    base, lean, full = side(runs["baseline"], "total"), side(runs["onecall"], "lean"), side(runs["onecall"], "with_clouds")
    res = {"mode": "ab", "pairs": pairs, "repeats": repeats, "rig": runs["baseline"][0]["rig"], "iters": runs["baseline"][0]["iters"],
           "points": runs["baseline"][0]["points"], "baseline_parent_library": base,
           "baseline_parts_ms": {k: side(runs["baseline"], k)["median_ms"] for k in ("radial", "vertices", "strip", "refine")},
           "onecall": lean, "onecall_with_clouds": full,
           "onecall_minus_baseline_ms": round(lean["median_ms"] - base["median_ms"], 4),
           "onecall_not_slower_beyond_baseline_spread": lean["median_ms"] <= base["median_ms"] + base["spread_ms"],
           "digests": sorted({x["digest"] for x in runs["baseline"]} | {x["digest"] for x in runs["onecall"]}),
           "poses_digests": sorted({x["poses_digest"] for x in runs["baseline"]} | {x["poses_digest"] for x in runs["onecall"]}),
           "kept_bytes": runs["onecall"][0]["kept_bytes"]}
    res["same_digest"] = len(res["digests"]) == 1 and len(res["poses_digests"]) == 1
    print(json.dumps(res))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--ab" in sys.argv:
        return ab(args[0], int(args[1]) if len(args) > 1 else 3, int(args[2]) if len(args) > 2 else 5)
    native.require_gpu()
    repeats = int(args[0]) if args else 5
    S, w, h = (int(x) for x in args[1:4]) if len(args) >= 4 else (8, 512, 424)
    iters = (int(args[4]), int(args[5])) if len(args) >= 6 else (2, 10)
    mode = plane if "--plane" in sys.argv else (baseline if "--baseline" in sys.argv else onecall)
    return mode(repeats, S, w, h, iters)


if __name__ == "__main__":
    main()
