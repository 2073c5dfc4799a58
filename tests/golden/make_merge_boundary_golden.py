#!/usr/bin/env python3
"""Regenerates tests/golden/merge_boundary_ref.npz: the reference's own generateMeshFromDepthMaps(bgenerate_triangles = true)
(src/NativeUtils/depthprocessing.cpp) on the rigs of tests/merge_boundary_cases.py.

    python tests/golden/make_merge_boundary_golden.py <LiveScan3D checkout> [output directory]

The reference is built as tests/golden/make_export_golden.py builds it (the same stand-ins and the same two text edits of a temporary
copy, which that script explains); nothing of it is kept -- only the results.  Per rig the fixture holds the sha256 of the rig's
inputs (the rigs are rebuilt by the tests, and must still be the ones the fixture was made from), the reference's triangles
int32 (m, 3) -- or, for merge_boundary_cases.DIGEST_ONLY, their sha256 and count, which keeps the file below the other fixtures --,
its vertex count and the per-sensor vertex offsets (generateVerticesFromDepthMap for every index)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_export_golden as meg  # noqa: E402
from tests import export_cases, merge_boundary_cases  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    outdir = sys.argv[2] if len(sys.argv) == 3 else HERE
    arrays = {"names": np.array(merge_boundary_cases.NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = meg.build(sys.argv[1], tmp)
        for name in merge_boundary_cases.NAMES:
            rig = merge_boundary_cases.rig(name)
            res = meg.call(exe, tmp, [(meg.OP_MESH, rig, 0, 1, 0), (meg.OP_MESH, rig, 0, 0, 0)] + [(meg.OP_VERTS, rig, 0, 0, i) for i in range(rig.n)])
            (v, tri), (v0, _) = res[0], res[1]
            assert v.tobytes() == v0.tobytes(), name          # the merge touches no vertex
            counts = [len(x) // 16 for x, _ in res[2:]]
            assert sum(counts) == len(v) // 16, name
            arrays[name + "/inputs"] = np.array(export_cases.sha(export_cases.rig_inputs(rig)))
            if name in merge_boundary_cases.DIGEST_ONLY:
                arrays[name + "/triangles_sha256"] = np.array(export_cases.sha(tri.astype("<i4")))
                arrays[name + "/n_triangles"] = np.int32(len(tri))
            else:
                arrays[name + "/triangles"] = tri.astype("<i4")
            arrays[name + "/n_vertices"] = np.int32(len(v) // 16)
            arrays[name + "/offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    np.savez_compressed(os.path.join(outdir, "merge_boundary_ref.npz"), **arrays)
    print(f"wrote {outdir}/merge_boundary_ref.npz: {len(merge_boundary_cases.NAMES)} rigs")


if __name__ == "__main__":
    main()
