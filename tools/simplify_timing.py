#!/usr/bin/env python3
"""Mesh level of detail (lsnFusionSimplify) on 8 x 512x424 ring-scene ticks, one tick and a batch of 8, cells 0.005 / 0.01 / 0.02 / 0.05:
one JSON line per configuration with

  us_per_call     HIP events round one call over all ticks (median of `reps`), table clear included
  kept            vertices out / vertices in, triangles out / triangles in (tick 0)
  bytes, floor_us the stage's algorithmic bytes (every array read or written once per pass that touches it, 12 B of table per vertex per
                  table pass, the table clear) and their time at the box's device-to-device copy rate, measured here

then, with --host, what a server pays per tick for the outbound stream: wall-clock ms and bytes of lsnLastMeshTransferFrame and, where the
library has it, lsnLastMeshTransferFrameLod(cell) on the same resident mesh.  With $LSN_NATIVE_LIB pointing at another build of the
library (the commit before the stage) the plain export of that build is what is measured.

    python tools/simplify_timing.py [reps] [--host] [--host-only]"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402

CELLS = (0.005, 0.01, 0.02, 0.05)


def copy_rate():
    """Device-to-device copy of 256 MiB: bytes moved (read + write) per second."""
    import torch
    x = torch.empty(1 << 28, dtype=torch.uint8, device="cuda").random_(0, 255)
    y = torch.empty_like(x)
    ms = timing.event_ms(lambda: y.copy_(x), 10, 2)
    return 2 * x.numel() / (ms * 1e-3)


def stage_bytes(cap, nv, nt, kept_v, kept_t):
    slots = 1
    while slots < 2 * cap:
        slots <<= 1
    clear = 12 * slots
    insert = 16 * nv + 12 * nv + 4 * nv                  # vertices in, key + value of the slot, the slot out
    lookup = 4 * nv + 4 * nv + 4 * nv                    # slot in, value in, representative out
    write = 4 * nv + 16 * kept_v * 2 + 4 * kept_v        # representative in, kept vertices in and out, output index out
    remap = 4 * nv + 4 * nv + 4 * nv + 4 * nv            # representative in, output index in, remap out twice (scratch and caller)
    tris = 2 * (12 * nt + 12 * nt) + 12 * kept_t         # two passes: indices in, three remap entries in; survivors out
    return clear + insert + lookup + write + remap + tris


def device_part(reps):
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rate = copy_rate()
    print(json.dumps({"copy_rate_TBps": round(rate / 1e12, 3)}), flush=True)
    stream = int(torch.cuda.current_stream().cuda_stream)
    for T in (1, 8):
        rigs = [synth.make_rig("scene", 8, tick=k) for k in range(T)]
        with DeviceFusion.from_rigs(rigs) as fus:
            fus.run_mesh()
            nv, nt = int(fus.host_offsets()[0, -1]), int(fus.host_tri_offsets()[0, -1])
            for cell in CELLS:
                v, off, t, toff, remap = fus.simplify(cell)          # the outputs, allocated outside the timed window
                call = lambda: fus.plan.simplify(cell, fus.vertices.data_ptr(), fus.offsets.data_ptr(), fus.triangles.data_ptr(),
                                                 fus.tri_offsets.data_ptr(), v.data_ptr(), off.data_ptr(), t.data_ptr(), toff.data_ptr(),
                                                 remap.data_ptr(), stream)
                ms = timing.event_ms(call, reps, 3)
                kv, kt = int(off[0, -1]), int(toff[0, -1])
                b = T * stage_bytes(fus.capacity, nv, nt, kv, kt)
                print(json.dumps({"ticks": T, "cell": cell, "us_per_call": round(ms * 1e3, 1), "vertices": nv, "triangles": nt,
                                  "kept_vertices": round(kv / max(nv, 1), 4), "kept_triangles": round(kt / max(nt, 1), 4), "bytes": b,
                                  "floor_us": round(b / rate * 1e6, 1), **fus.plan.simplify_diagnostics(0)}), flush=True)


def host_part(reps):
    rig = synth.make_rig("scene", 8)
    v, t = native.generate_mesh_from_depth_maps(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    L = native.lib()

    def measure(fn, label, cell=None):
        cap = fn(None, 0)
        out = np.zeros(cap, np.uint8)
        ms, n = [], 0
        for _ in range(reps + 3):
            t0 = time.perf_counter()
            n = fn(out.ctypes.data, cap)
            ms.append((time.perf_counter() - t0) * 1e3)
        assert n >= 0, native.last_error()
        print(json.dumps({"export": label, "cell": cell, "library": os.environ.get("LSN_NATIVE_LIB", "tree"), "vertices": len(v), "triangles": len(t),
                          "ms_per_call": round(statistics.median(ms[3:]), 3), "stream_bytes": int(n)}), flush=True)

    measure(L.lsnLastMeshTransferFrame, "lsnLastMeshTransferFrame")
    if hasattr(L, "lsnLastMeshTransferFrameLod"):
        for cell in (0.0,) + CELLS:
            measure(lambda out, cap, c=cell: L.lsnLastMeshTransferFrameLod(c, out, cap), "lsnLastMeshTransferFrameLod", cell)


def main():
    args = sys.argv[1:]
    nums = [a for a in args if a.isdigit()]
    reps = int(nums[0]) if nums else 30
    native.require_gpu()
    if "--host-only" not in args:
        device_part(reps)
    if "--host" in args or "--host-only" in args:
        host_part(reps)


if __name__ == "__main__":
    main()
