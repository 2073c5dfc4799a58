#!/usr/bin/env python3
"""Mesh smoothing (lsnFusionSmooth) on 8 x 512x424 ring-scene ticks, one tick and a batch of 8, for the plain mesh and for the outputs of
simplify(0.01), open vertices pinned: one JSON line per configuration with

  call_1_us       HIP events round one lsnFusionSmooth(1, 0.5, -0.53) over all ticks (median of `reps`): clear, topology, flags, 2 passes
  call_10_us      the same with 10 iterations: 20 passes
  pass_us         (call_10_us - call_1_us) / 18: one pass, scatter + finish, as the calls pay for it
  fixed_us        call_1_us - 2 pass_us: the clear, the topology pass and the flags
  free_10_us      10 iterations with pin_boundary = 0: no topology pass
  face_us         nm_face_kernel on the same mesh in the same run, from the plan's own event pair (lsnFusionProfile / lsnFusionKernelStats;
                  mean over the calls): the yardstick, a scatter of the same shape (nine 64-bit adds per triangle, no counts)
  normals_call_us one lsnFusionNormals: clear + face pass + finish, the three launches a smoothing pass compares with
  add_bytes       per pass, 72 B (nine 64-bit adds) + 12 B (three 32-bit adds) per used triangle over all ticks, an upper bound

    python tools/smooth_timing.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402


def measure(fus, label, v, off, t, toff, reps, stream):
    import torch
    out = fus.smooth(10, 0.5, -0.53, True, v, off, t, toff)          # the output and the scratch, allocated outside the timed window
    nrm = fus.normals(v, off, t, toff)
    call = lambda it, pin: fus.plan.smooth(it, 0.5, -0.53, pin, v.data_ptr(), off.data_ptr(), t.data_ptr(), toff.data_ptr(), out.data_ptr(), stream)
    call_1 = timing.event_ms(lambda: call(1, True), reps, 3) * 1e3
    call_10 = timing.event_ms(lambda: call(10, True), reps, 3) * 1e3
    free_10 = timing.event_ms(lambda: call(10, False), reps, 3) * 1e3
    call(10, True)
    used = sum(fus.plan.smooth_diagnostics(k)["used"] for k in range(fus.n_ticks))
    d0 = fus.plan.smooth_diagnostics(0)
    normals = lambda: fus.plan.normals(v.data_ptr(), off.data_ptr(), t.data_ptr(), toff.data_ptr(), nrm.data_ptr(), stream)
    normals_call = timing.event_ms(normals, reps, 3) * 1e3
    fus.plan.kernel_stats(reset=True)
    fus.plan.profile(True)
    for _ in range(reps):
        normals()
    torch.cuda.synchronize()
    face = fus.plan.kernel_stats(reset=True)
    fus.plan.profile(False)
    pass_us = (call_10 - call_1) / 18
    return {"mesh": label, "ticks": fus.n_ticks, "vertices": int(off[0, -1]), "triangles": int(toff[0, -1]), "call_1_us": round(call_1, 1),
            "call_10_us": round(call_10, 1), "pass_us": round(pass_us, 1), "fixed_us": round(call_1 - 2 * pass_us, 1), "free_10_us": round(free_10, 1),
            "timed_kernel": face["kernel"], "face_us": round(face["avg_ms"] * 1e3, 1), "normals_call_us": round(normals_call, 1),
            "add_bytes": 84 * used, **d0}


def main():
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    nums = [a for a in sys.argv[1:] if a.isdigit()]
    reps = int(nums[0]) if nums else 30
    native.require_gpu()
    stream = int(torch.cuda.current_stream().cuda_stream)
    for T in (1, 8):
        rigs = [synth.make_rig("scene", 8, tick=k) for k in range(T)]
        with DeviceFusion.from_rigs(rigs) as fus:
            fus.run_mesh()
            print(json.dumps(measure(fus, "plain", fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, reps, stream)), flush=True)
            v, off, t, toff, _ = fus.simplify(0.01)
            print(json.dumps(measure(fus, "simplify(0.01)", v, off, t, toff, reps, stream)), flush=True)


if __name__ == "__main__":
    main()
