#!/usr/bin/env python3
"""The fragment filter (lsnFusionFragments) on one 8 x 512x424 ring-scene tick, min_vertices 2 / 64 / 1024 and off (1), beside
lsnFusionSimplify(0.01) and lsnFusionNormals on the same mesh: one JSON line per configuration with

  us_per_call     HIP events round one call (median of `reps` after 3 warm-up calls)
  removed         vertices removed / vertices in, triangles dropped / triangles in, the components and the removed ones
  launches        kernels per call: 11 + the pointer-doubling launches, ceil(log2(capacity)); 8 when off
  bytes, floor_us the stage's algorithmic bytes (every array read or written once per pass that touches it; a pointer-doubling launch
                  reads parent twice and, at most, writes it once) and their time at the box's device-to-device copy rate, measured here
  of_copy_rate    floor_us / us_per_call

    python tools/fragments_timing.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tools import timing  # noqa: E402
from tools.simplify_timing import copy_rate  # noqa: E402

MINS = (2, 64, 1024, 1)


def jump_launches(cap):
    k = 0
    while (1 << k) < cap:
        k += 1
    return k


def stage_bytes(cap, nv, nt, kept_v, kept_t, off):
    compaction = (4 * nv                                   # keep: the flag out ...
                  + 4 * nv + 2 * 16 * kept_v + 4 * nv + 4 * nv      # write: flag in, kept vertices in and out, output index and remap out
                  + 2 * 12 * nt + 12 * kept_t)             # two triangle passes: indices in; survivors out
    if off:
        return compaction
    init = 8 * nv                                          # parent and size out
    union = 12 * nt + 2 * 3 * 4 * nt                       # indices in; a parent and a grandparent per corner, at least
    jumps = jump_launches(cap) * 12 * nv                   # parent, parent's parent in, parent out
    sizes = 4 * nv                                         # labels in (the adds: one per run)
    keep = 8 * nv                                          # label and its size in
    labels = 8 * nv                                        # label in, label out
    remap = 2 * 12 * nt                                    # three remap entries per triangle, two passes
    return init + union + jumps + sizes + keep + labels + remap + compaction


def main():
    nums = [a for a in sys.argv[1:] if a.isdigit()]
    reps = int(nums[0]) if nums else 30
    native.require_gpu()
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    rate = copy_rate()
    print(json.dumps({"copy_rate_TBps": round(rate / 1e12, 3)}), flush=True)
    stream = int(torch.cuda.current_stream().cuda_stream)
    with DeviceFusion.from_rigs([synth.make_rig("scene", 8)]) as fus:
        fus.run_mesh()
        nv, nt = int(fus.host_offsets()[0, -1]), int(fus.host_tri_offsets()[0, -1])
        ins = (fus.vertices.data_ptr(), fus.offsets.data_ptr(), fus.triangles.data_ptr(), fus.tri_offsets.data_ptr())
        for m in MINS:
            v, off, t, toff, remap, labels = fus.fragments(m)          # the outputs, allocated outside the timed window
            call = lambda: fus.plan.fragments(m, *ins, v.data_ptr(), off.data_ptr(), t.data_ptr(), toff.data_ptr(), remap.data_ptr(),
                                              labels.data_ptr(), stream)
            ms = timing.event_ms(call, reps, 3)
            kv, kt = int(off[0, -1]), int(toff[0, -1])
            b = stage_bytes(fus.capacity, nv, nt, kv, kt, m <= 1)
            floor = b / rate * 1e6
            print(json.dumps({"stage": "fragments", "min_vertices": m, "us_per_call": round(ms * 1e3, 1), "vertices": nv, "triangles": nt,
                              "removed_vertex_share": round(1 - kv / max(nv, 1), 4), "dropped_triangle_share": round(1 - kt / max(nt, 1), 4),
                              "launches": 8 if m <= 1 else 11 + jump_launches(fus.capacity), "bytes": b, "floor_us": round(floor, 1),
                              "of_copy_rate": round(floor / (ms * 1e3), 3), **fus.plan.fragments_diagnostics(0)}), flush=True)
        sv, soff, st, stoff, sremap = fus.simplify(0.01)
        ms = timing.event_ms(lambda: fus.plan.simplify(0.01, *ins, sv.data_ptr(), soff.data_ptr(), st.data_ptr(), stoff.data_ptr(),
                                                       sremap.data_ptr(), stream), reps, 3)
        print(json.dumps({"stage": "simplify", "cell": 0.01, "us_per_call": round(ms * 1e3, 1), "vertices": nv, "triangles": nt}), flush=True)
        normals = fus.normals()
        ms = timing.event_ms(lambda: fus.plan.normals(*ins, normals.data_ptr(), stream), reps, 3)
        print(json.dumps({"stage": "normals", "us_per_call": round(ms * 1e3, 1), "vertices": nv, "triangles": nt}), flush=True)


if __name__ == "__main__":
    main()
