#!/usr/bin/env python3
"""Regenerates tests/golden/flying_pixels_ref.npz and flying_pixels_digests.json: the reference's own flying-pixel filter, the live
three-argument KinectCapture::filterFlyingPixels (src/LiveScanClient/kinectCapture.cpp:132-174; the two-argument one above it sits
inside a comment), run on fixed depth maps.

    python tests/golden/make_flying_golden.py <LiveScan3D checkout>

kinectCapture.cpp includes the Kinect SDK, so the function is cut out of it by name and compiled with g++ on x86-64 (-O2
-ffp-contract=off, like the reference's /fp:precise) behind a stand-in KinectCapture that has only pDepth, nDepthFrameWidth and
nDepthFrameHeight, together with a small driver, and run; nothing of the reference is kept -- only inputs and results.

Frames and settings: tests/flying_cases.py.  Every case runs with the third argument at 0, 4 and 1000 and the three maps must be
identical (the reference overwrites the argument before it reads it); `third_argument_ignored` records that they were.  Small frames are
kept in full (input once per frame, result per case); the 512 x 424 and 1024 x 1024 frames are regenerated from livescan3d_amd/synth.py
and pinned by sha256 of input and result, with their valid and removed pixel counts, in the .json.  The generator also checks that the
two-level frames tell the filter from a pass that sees its own zeros."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "flying_pixels_ref.npz")
OUT_JSON = os.path.join(ROOT, "tests", "golden", "flying_pixels_digests.json")

STANDIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef unsigned short UINT16;
class KinectCapture {
public:
    UINT16 *pDepth;
    int nDepthFrameWidth, nDepthFrameHeight;
    void filterFlyingPixels(int neighbourhoodSize, float thr, int maxNonFittingNeighbours);
};
"""

DRIVER = r"""
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) exit(2); }
int main(int argc, char **argv)
{
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int n_cases;
    rd(&n_cases, 4, in);
    for (int c = 0; c < n_cases; c++) {
        int w, h, r, thr, third;
        rd(&w, 4, in); rd(&h, 4, in); rd(&r, 4, in); rd(&thr, 4, in); rd(&third, 4, in);
        std::vector<UINT16> d((size_t)w * h);
        rd(d.data(), 2 * d.size(), in);
        KinectCapture k;
        k.pDepth = d.data();
        k.nDepthFrameWidth = w;
        k.nDepthFrameHeight = h;
        k.filterFlyingPixels(r, (float)thr, third);   // as AcquireFrame calls it (kinectCapture.cpp:198-199)
        fwrite(d.data(), 2, d.size(), out);
    }
    fclose(out);
    return 0;
}
"""

FUNCTION = r"void KinectCapture::filterFlyingPixels\(int \w+, float \w+, int \w+\)"


def cut(source, pattern):
    """The definition that starts at the line matching `pattern`, to its matching closing brace."""
    m = re.search(r"^" + pattern, source, re.M)
    assert m, pattern
    i = source.index("{", m.start())
    depth = 0
    for j in range(i, len(source)):
        depth += {"{": 1, "}": -1}.get(source[j], 0)
        if depth == 0:
            return source[m.start():j + 1] + "\n"
    raise ValueError(pattern)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u2").tobytes()).hexdigest()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from tests import flying_cases, flying_ref
    ref = sys.argv[1]
    src = open(os.path.join(ref, "src", "LiveScanClient", "kinectCapture.cpp"), encoding="utf-8", errors="replace").read()
    frames = flying_cases.small_frames()
    small = flying_cases.small_cases(frames)
    big = flying_cases.digest_cases()
    big_frames = {}
    for spec, _, _ in big:
        key = json.dumps(spec, sort_keys=True)
        if key not in big_frames:
            big_frames[key] = flying_cases.digest_frame(spec)
    runs = [(frames[name], r, t) for name, r, t in small] + [(big_frames[json.dumps(sp, sort_keys=True)], r, t) for sp, r, t in big]
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(drv, "w") as f:
            f.write(STANDIN + cut(src, FUNCTION) + DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", drv, "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.int32(len(runs) * len(flying_cases.THIRD_ARGUMENTS)).tobytes())
            for d, r, t in runs:
                for third in flying_cases.THIRD_ARGUMENTS:
                    f.write(np.int32([d.shape[1], d.shape[0], r, t, third]).tobytes() + np.ascontiguousarray(d, dtype="<u2").tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    results, ignored, pos = [], [], 0
    for d, r, t in runs:
        maps = []
        for _ in flying_cases.THIRD_ARGUMENTS:
            maps.append(np.frombuffer(raw[pos:pos + 2 * d.size], "<u2").reshape(d.shape).copy())
            pos += 2 * d.size
        ignored.append(all(m.tobytes() == maps[0].tobytes() for m in maps))
        results.append(maps[0])
    assert pos == len(raw)
    assert all(ignored), "the third argument changed a result"
    arrays = {"frame_names": np.array(list(frames))}
    for name, d in frames.items():
        arrays[f"frame_{name}"] = d
    names = list(frames)
    for c, (name, r, t) in enumerate(small):
        arrays[f"result_{c}"] = results[c]
    arrays["case_frame"] = np.int32([names.index(n) for n, _, _ in small])
    arrays["case_r"] = np.int32([r for _, r, _ in small])
    arrays["case_thr"] = np.int32([t for _, _, t in small])
    arrays["third_arguments"] = np.int32(flying_cases.THIRD_ARGUMENTS)
    arrays["third_argument_ignored"] = np.array(ignored[:len(small)])
    # the cases that show that decisions are taken on the unmodified map: a pass that zeroes as it scans gives another result
    for name in ("two_levels_37x29", "two_levels_holes_37x29"):
        c = small.index((name, 1, 20))
        assert flying_ref.filter_in_place_sequential(frames[name], 1, 20).tobytes() != results[c].tobytes(), name
    np.savez_compressed(OUT, **arrays)
    entries = []
    for k, (spec, r, t) in enumerate(big):
        d, res = big_frames[json.dumps(spec, sort_keys=True)], results[len(small) + k]
        entries.append({"frame": spec, "r": r, "thr": t, "input_sha256": sha(d), "result_sha256": sha(res), "valid": int((d != 0).sum()),
                        "removed": int(((d != 0) & (res == 0)).sum()), "third_argument_ignored": bool(ignored[len(small) + k])})
    with open(OUT_JSON, "w") as f:
        json.dump({"third_arguments": list(flying_cases.THIRD_ARGUMENTS), "cases": entries}, f, indent=1)
        f.write("\n")
    print(f"wrote {OUT}: {len(names)} frames, {len(small)} cases, {os.path.getsize(OUT)} bytes; {OUT_JSON}: {len(entries)} cases")


if __name__ == "__main__":
    main()
