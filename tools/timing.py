"""The two timing loops of the tools (the protocol behind profiles/*_timing.txt): HIP events round a device call, wall clock round a
C-ABI export call.  Every tool passes its own repeat and warm-up counts."""
import ctypes as C
import statistics
import time

from livescan3d_amd import native


def event_ms(fn, reps, warmup=2, before=None):
    """Median ms of `reps` runs of fn() between two HIP events on the current stream, after `warmup` runs that are dropped; the device is
    synchronised after every run.  before(): untimed work ahead of every run (a refill of what fn changes in place)."""
    import torch
    ms = []
    for _ in range(reps + warmup):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[warmup:])


def export_call_ms(call, calls, warmup=3, frames=None):
    """Wall-clock ms of each of `calls` runs of call(byref(mesh), *frames()) + deleteMesh (what LiveScanServer pays per tick before its own
    copy), after `warmup` runs that are dropped.  frames(): untimed, a fresh copy of what the export writes back into."""
    L = native.lib()
    t = []
    for _ in range(calls + warmup):
        args = frames() if frames is not None else ()
        m = native.Mesh()
        t0 = time.perf_counter()
        call(C.byref(m), *args)
        L.deleteMesh(C.byref(m))
        t.append((time.perf_counter() - t0) * 1e3)
    return t[warmup:]


def rig_pointers(rig, depth_maps=None, depth_colors=None):
    """The leading arguments of the merge exports for a rig: (n, depth maps, colours, widths, heights, intr, wt) as pointers, and its
    bounds as six floats."""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    dm = rig.depth_maps if depth_maps is None else depth_maps
    dc = rig.depth_colors if depth_colors is None else depth_colors
    return (rig.n, p(dm), p(dc), p(rig.widths), p(rig.heights), p(rig.intr), p(rig.wt)), [float(x) for x in rig.bounds]
