#!/usr/bin/env python3
"""Vertex normals (lsnFusionNormals) on 8 x 512x424 ring-scene ticks, one tick and a batch of 8, for the plain mesh and for the outputs of
simplify(0.01): one JSON line per configuration with

  run_mesh_us     HIP events round lsnFusionRunMesh on the same ticks (median of `reps`): what building the mesh costs
  call_us         HIP events round one lsnFusionNormals over all ticks: clear + face pass + finish
  face_us         nm_face_kernel alone, from the plan's own event pair (lsnFusionProfile / lsnFusionKernelStats; mean over the calls)
  rest_us         one lsnFusionNormals with every triangle count set to 0: clear + an empty face pass + finish, i.e. what is not the adds
  add_bytes       72 B (nine 64-bit adds) per used triangle over all ticks, an upper bound (adds of 0 are skipped), and add_GBps, those
                  bytes over face_us

    python tools/normals_timing.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402


def measure(fus, label, v, off, t, toff, reps, stream):
    import torch
    out = fus.normals(v, off, t, toff)                      # the output and the scratch, allocated outside the timed window
    call = lambda tri_off=toff: fus.plan.normals(v.data_ptr(), off.data_ptr(), t.data_ptr(), tri_off.data_ptr(), out.data_ptr(), stream)
    call_ms = timing.event_ms(call, reps, 3)
    used = sum(fus.plan.normals_diagnostics(k)["used"] for k in range(fus.n_ticks))
    d0 = fus.plan.normals_diagnostics(0)
    fus.plan.kernel_stats(reset=True)
    fus.plan.profile(True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    face = fus.plan.kernel_stats(reset=True)
    fus.plan.profile(False)
    none = torch.zeros_like(toff)
    rest_ms = timing.event_ms(lambda: call(none), reps, 3)
    face_us = face["avg_ms"] * 1e3
    return {"mesh": label, "ticks": fus.n_ticks, "vertices": int(off[0, -1]), "triangles": int(toff[0, -1]), "call_us": round(call_ms * 1e3, 1),
            "timed_kernel": face["kernel"], "face_us": round(face_us, 1), "rest_us": round(rest_ms * 1e3, 1), "add_bytes": 72 * used,
            "add_GBps": round(72 * used / max(face_us, 1e-3) / 1e3, 1), **d0}


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
            run_mesh_us = round(timing.event_ms(fus.run_mesh, reps, 3) * 1e3, 1)
            row = measure(fus, "plain", fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, reps, stream)
            print(json.dumps({**row, "run_mesh_us": run_mesh_us}), flush=True)
            v, off, t, toff, _ = fus.simplify(0.01)
            row = measure(fus, "simplify(0.01)", v, off, t, toff, reps, stream)
            print(json.dumps({**row, "run_mesh_us": run_mesh_us}), flush=True)


if __name__ == "__main__":
    main()
