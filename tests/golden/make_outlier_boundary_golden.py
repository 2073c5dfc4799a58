#!/usr/bin/env python3
"""Regenerates tests/golden/outlier_boundary_ref.npz: the reference's own KNNeighbors and filter() (src/LiveScanClient/filter.cpp:19-81,
over include/LiveScanClient/filter.h and include/nanoflann.h) on every (tick, sensor) block of every case of
tests/outlier_boundary_cases.py.

    python tests/golden/make_outlier_boundary_golden.py <LiveScan3D checkout> [output directory]

The reference is cut out and compiled as tests/golden/make_outlier_golden.py does it (the same stand-in utils.h, the same driver, g++ -O2
-ffp-contract=off), which that script explains; nothing of the reference is kept -- only the results.  Stored, all blocks one after the
other: the cases' names, frames, k and maxDist; per block its case, tick, sensor and size; the points as they went in; and what came
out: changedVerticesMap (its values for the keys 0 .. n-1; key -1 maps to -1 everywhere) and KNNeighbors' kDistance of every point."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_outlier_golden as mog  # noqa: E402
from tests import outlier_boundary_cases as cases  # noqa: E402


def build(ref, tmp):
    src = open(os.path.join(ref, "src", "LiveScanClient", "filter.cpp"), encoding="utf-8", errors="replace").read()
    shutil.copy(os.path.join(ref, "include", "LiveScanClient", "filter.h"), os.path.join(tmp, "filter.h"))
    with open(os.path.join(tmp, "utils.h"), "w") as f:
        f.write(mog.UTILS_STANDIN)
    drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
    with open(drv, "w") as f:
        f.write('#include "filter.h"\n#include <unordered_map>\nusing namespace std;\n' + "".join(mog.cut(src, p) for p in mog.FUNCTIONS) + mog.DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I", tmp, "-I", os.path.join(ref, "include"), drv, "-o", exe])
    return exe


def run(exe, tmp, jobs):
    """jobs: [(points (n, 3) float32, k >= 1, maxDist > 0)] -> [(kDistance float32[n], changedVerticesMap's values int32[n])]."""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(jobs)).tobytes())
        for pts, k, d in jobs:
            f.write(np.int32([len(pts), k]).tobytes() + np.float32(d).tobytes() + pts.tobytes() + np.zeros((len(pts), 4), np.uint8).tobytes())
    subprocess.check_call([exe, fin, fout])
    raw, pos, out = open(fout, "rb").read(), 0, []
    for pts, k, d in jobs:
        n = len(pts)
        kd = np.frombuffer(raw[pos:pos + 4 * n], "<f4").copy()
        pos += 4 * n
        nv = int(np.frombuffer(raw[pos:pos + 4], "<i4")[0])
        pos += 4 + 16 * nv
        nm = int(np.frombuffer(raw[pos:pos + 4], "<i4")[0])
        pos += 4
        kv = np.frombuffer(raw[pos:pos + 8 * nm], "<i4").reshape(-1, 2)
        pos += 8 * nm
        assert nm == n + 1 and kv[0].tolist() == [-1, -1] and np.array_equal(kv[1:, 0], np.arange(n)), (n, k, d)
        changed = kv[1:, 1].astype(np.int32)
        assert nv == int((changed >= 0).sum())
        out.append((kd, changed))
    assert pos == len(raw)
    return out


def layout():
    """What the fixture says about the cases themselves (tests/test_outlier_boundary_ref.py holds the committed file to it)."""
    blocks = [(i, t, s, b) for i, c in enumerate(cases.CASES) for t, s, b in c.blocks()]
    return {"case_names": np.array(cases.NAMES), "case_k": np.int32([c.k for c in cases.CASES]),
            "case_max_dist": np.float32([c.max_dist for c in cases.CASES]),
            "case_n_frames": np.int32([len(c.frames) for c in cases.CASES]),
            "case_frames": np.int32([wh for c in cases.CASES for wh in c.frames]).reshape(-1, 2),
            "block_case": np.int32([i for i, _, _, _ in blocks]), "block_tick": np.int32([t for _, t, _, _ in blocks]),
            "block_sensor": np.int32([s for _, _, s, _ in blocks]), "block_n": np.int32([len(b) for _, _, _, b in blocks]),
            "points": np.concatenate([b for _, _, _, b in blocks]).astype(np.float32)}


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    outdir = sys.argv[2] if len(sys.argv) == 3 else HERE
    arrays = layout()
    jobs = [(b, c.k, c.max_dist) for c in cases.CASES for _, _, b in c.blocks()]
    with tempfile.TemporaryDirectory() as tmp:
        results = run(build(sys.argv[1], tmp), tmp, jobs)
    arrays["kdist"] = np.concatenate([kd for kd, _ in results]).astype(np.float32)
    arrays["changed"] = np.concatenate([ch for _, ch in results]).astype(np.int32)
    out = os.path.join(outdir, "outlier_boundary_ref.npz")
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(cases.CASES)} cases, {len(jobs)} blocks, {len(arrays['points'])} points, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
