#!/usr/bin/env python3
"""Regenerates tests/golden/color_boundary_ref.npz: the reference's own generateMeshFromDepthMaps(bcolor_transfer = true)
(src/NativeUtils/depthprocessing.cpp) on the rigs of tests/color_boundary_cases.py.

    python tests/golden/make_color_boundary_golden.py <LiveScan3D checkout> [output directory]

The reference is built as tests/golden/make_export_golden.py builds it (the same stand-ins and the same two text edits of a temporary
copy, which that script explains); nothing of it is kept -- only the results.  Per rig the fixture holds the sha256 of the rig's
inputs (the rigs are rebuilt by the tests, and must still be the ones the fixture was made from), the number of vertices and the
sha256 of the corrected vertex bytes -- and, for color_boundary_cases.FULL, the bytes themselves, uint8 (n, 16); digests for the rest
keep the file below the other fixtures.  The rigs of color_boundary_cases.DEFINED are left out: there the reference reads
colors1[-3..-1], and the restatements (tests/color_ref.py, tests/color_ref_py.py) are the definition."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_export_golden as meg  # noqa: E402
from tests import color_boundary_cases as cases, export_cases  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    outdir = sys.argv[2] if len(sys.argv) == 3 else HERE
    names = [n for n in cases.NAMES if n not in cases.DEFINED]
    arrays = {"names": np.array(names)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = meg.build(sys.argv[1], tmp)
        for name in names:
            rig = cases.rig(name)
            (v, tri), (v0, tri0) = meg.call(exe, tmp, [(meg.OP_MESH, rig, 1, 0, 0), (meg.OP_MESH, rig, 0, 0, 0)])
            assert len(v) == len(v0) and tri.tobytes() == tri0.tobytes(), name
            a, b = v.reshape(-1, 16), v0.reshape(-1, 16)
            assert a[:, 3:].tobytes() == b[:, 3:].tobytes(), name          # the transfer touches the colour bytes alone
            arrays[name + "/inputs"] = np.array(export_cases.sha(export_cases.rig_inputs(rig)))
            arrays[name + "/n_vertices"] = np.int32(len(a))
            arrays[name + "/vertices_sha256"] = np.array(export_cases.sha(a))
            arrays[name + "/changed"] = np.int32((a[:, :3] != b[:, :3]).any(axis=1).sum())
            if name in cases.FULL:
                arrays[name + "/vertices"] = a
    np.savez_compressed(os.path.join(outdir, "color_boundary_ref.npz"), **arrays)
    print(f"wrote {outdir}/color_boundary_ref.npz: {len(names)} rigs")


if __name__ == "__main__":
    main()
