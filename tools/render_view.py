#!/usr/bin/env python3
"""Render view (lsnFusionRenderViews) on one tick of the 8 x 512x424 ring scene, from a pose half-way between ring sensors 0 and 1: mesh
and points mode, 512x424 and 1024x1024 views, at the sensors' focal length and zoomed in 4x.  Prints one JSON line per configuration:

  ms_per_view     HIP events round one call of one view (median of `reps`)
  drawn / large   primitives drawn; triangles whose bounding box went through the work list (one wave per triangle), and their share
  pixels          pixels with depth != 0

and writes the mesh view at 512x424, sensors' focal length, as a binary PPM.

    python tools/render_view.py [reps] [--ppm PATH]"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from livescan3d_amd import native, synth  # noqa: E402
from tests import render_ref  # noqa: E402
from tools import timing  # noqa: E402


def main():
    args = sys.argv[1:]
    ppm = args[args.index("--ppm") + 1] if "--ppm" in args else "render_view.ppm"
    nums = [a for a in args if a.isdigit()]
    reps = int(nums[0]) if nums else 100
    native.require_gpu()
    from livescan3d_amd.fusion import DeviceFusion
    rig = synth.make_rig("scene", 8)
    view = render_ref.pose_between(rig.wt[0:12], rig.wt[12:24])
    focal = float(rig.intr[2])
    import torch
    stream = int(torch.cuda.current_stream().cuda_stream)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        nv, nt = int(fus.host_offsets()[0, -1]), int(fus.host_tri_offsets()[0, -1])
        print(json.dumps({"rig": "8 x 512x424 ring scene, one tick", "vertices": nv, "triangles": nt, "reps": reps}))
        for points in (False, True):
            for w, h in ((512, 424), (1024, 1024)):
                for zoom in (1, 4):
                    intr = np.array([(w - 1) / 2.0, (h - 1) / 2.0, focal * zoom, focal * zoom, 0, 0, 0], dtype=np.float32)
                    depth, rgb = fus.render_views(intr, view, w, h, points=points)      # the outputs, allocated outside the timed window
                    tri = (0, 0) if points else (fus.triangles.data_ptr(), fus.tri_offsets.data_ptr())
                    ms = timing.event_ms(lambda: fus.plan.render_views(intr, view, w, h, fus.vertices.data_ptr(), fus.offsets.data_ptr(), *tri,
                                                                       depth.data_ptr(), rgb.data_ptr(), stream), reps, 3)
                    d = fus.plan.render_diagnostics(0, 0)
                    print(json.dumps({"mode": "points" if points else "mesh", "size": f"{w}x{h}", "zoom": zoom, "ms_per_view": round(ms, 4),
                                      "drawn": d["drawn"], "large": d["large"], "large_share": round(d["large"] / max(d["drawn"], 1), 4),
                                      "pixels": d["pixels"]}), flush=True)
                    if not points and (w, zoom) == (512, 1):
                        with open(ppm, "wb") as f:
                            f.write(b"P6\n%d %d\n255\n" % (w, h) + rgb[0, 0].cpu().numpy().tobytes())


if __name__ == "__main__":
    main()
