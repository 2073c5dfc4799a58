#!/usr/bin/env python3
"""Regenerates tests/golden/radial_boundary_ref.npz: the reference's own depthMapAndColorSetRadialCorrection
(src/NativeUtils/depthprocessing.cpp) on the cases of tests/radial_cases.py.

    python tests/golden/make_radial_boundary_golden.py <LiveScan3D checkout> [output directory]

The reference is built as tests/golden/make_export_golden.py builds it (the same stand-ins and the same two text edits of a temporary
copy, which that script explains); nothing of it is kept -- only the results.  Per case the fixture holds the sha256 of the case's
inputs (the cases are rebuilt by the tests, and must still be the ones the fixture was made from) and, tick after tick, the corrected
depth maps (u16) and colours -- or, for the cases of more than radial_cases.FULL_OUTPUT_PIXELS pixels, their sha256."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_export_golden as meg  # noqa: E402
from tests import export_cases, radial_cases  # noqa: E402


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    outdir = sys.argv[2] if len(sys.argv) == 3 else HERE
    arrays = {"names": np.array(radial_cases.NAMES)}
    with tempfile.TemporaryDirectory() as tmp:
        exe = meg.build(sys.argv[1], tmp)
        for name in radial_cases.NAMES:
            res = meg.call(exe, tmp, [(meg.OP_RADIAL, rig, 0, 0, 0) for rig in radial_cases.ticks(name)])
            depth, colors = np.concatenate([d for d, _ in res]).view("<u2"), np.concatenate([c for _, c in res])
            arrays[name + "/inputs"] = np.array(export_cases.sha(radial_cases.case_inputs(name)))
            if radial_cases.digest_only(name):
                arrays[name + "/depth_sha256"], arrays[name + "/colors_sha256"] = np.array(export_cases.sha(depth)), np.array(export_cases.sha(colors))
            else:
                arrays[name + "/depth"], arrays[name + "/colors"] = depth, colors
    np.savez_compressed(os.path.join(outdir, "radial_boundary_ref.npz"), **arrays)
    print(f"wrote {outdir}/radial_boundary_ref.npz: {len(radial_cases.NAMES)} cases")


if __name__ == "__main__":
    main()
