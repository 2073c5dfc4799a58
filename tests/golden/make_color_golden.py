#!/usr/bin/env python3
"""Regenerates tests/golden/color_transfer_ref.npz: the reference's own getColorCorrectionTransform + applyColorCorrection
(src/NativeUtils/colorcorrection.cpp, CS_RGB) run on fixed sample sets.

    python tests/golden/make_color_golden.py <LiveScan3D checkout>

The reference file is compiled in a temporary directory together with a small driver written here (it needs its header alone -- and <cmath>, which MSVC pulls in implicitly -- so it
builds on Linux); nothing of it is kept -- only the results.  The sets cover random sizes, the empty set, single samples, constant
colours (scale ~ 1e15, where the double -> int conversion of applyColorCorrection goes out of range) and every value of every channel.
Each case stores src / dst (n, 3) u8, the 9 doubles of the transform {mean_a1, mean_b1, mean_c1, mean_a2, mean_b2, mean_c2, std_scale_a,
std_scale_b, std_scale_c} and the 256 x 3 "every value" image after applyColorCorrection.  For the empty set the reference leaves
color_space uninitialised (colorcorrection.cpp:8-11); the driver sets CS_RGB there, which is the behaviour this project defines."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "color_transfer_ref.npz")

DRIVER = r"""
#include "colorcorrection.h"
#include <cstdio>
#include <vector>
int main(int argc, char **argv)
{
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    int n_cases = 0;
    if (!in || !out || fread(&n_cases, 4, 1, in) != 1) return 1;
    for (int c = 0; c < n_cases; c++) {
        int n = 0;
        if (fread(&n, 4, 1, in) != 1) return 1;
        std::vector<unsigned char> src(3 * (size_t)n), dst(3 * (size_t)n), img(256 * 3);
        if (n > 0 && (fread(src.data(), 1, src.size(), in) != src.size() || fread(dst.data(), 1, dst.size(), in) != dst.size())) return 1;
        ColorCorrectionParams p = getColorCorrectionTransform(src, dst, CS_RGB);
        if (n == 0) p.color_space = CS_RGB;
        const double v[9] = {p.mean_a1, p.mean_b1, p.mean_c1, p.mean_a2, p.mean_b2, p.mean_c2, p.std_scale_a, p.std_scale_b, p.std_scale_c};
        fwrite(v, sizeof(double), 9, out);
        for (int i = 0; i < 256; i++) img[3 * i] = img[3 * i + 1] = img[3 * i + 2] = (unsigned char)i;
        applyColorCorrection(img, p);
        fwrite(img.data(), 1, img.size(), out);
    }
    fclose(out);
    return 0;
}
"""


def cases():
    rng = np.random.default_rng(20261015)
    out = []
    for n in (1, 2, 3, 17, 1000, 65537):
        out.append((rng.integers(0, 256, (n, 3)), rng.integers(0, 256, (n, 3))))
    out.append((np.zeros((0, 3)), np.zeros((0, 3))))                                     # empty
    out.append((np.array([[10, 200, 30]]), np.array([[40, 50, 60]])))                     # single sample
    out.append((rng.integers(0, 256, (500, 3)), np.full((500, 3), 77)))                   # constant j: scale ~ 1e15
    out.append((np.full((500, 3), 140), rng.integers(0, 256, (500, 3))))                  # constant i: scale ~ 1e-15
    out.append((np.full((64, 3), 3), np.full((64, 3), 250)))                              # both constant
    a = rng.integers(0, 256, (4096, 3))
    out.append((a, np.clip(a * 0.8 + 20, 0, 255).astype(np.int64)))                       # a gain and an offset (the rig case)
    base = np.repeat(np.arange(256)[:, None], 3, axis=1)
    out.append((base[::-1].copy(), base.copy()))                                          # every value of every channel
    return [(s.astype(np.uint8), d.astype(np.uint8)) for s, d in out]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src_dir = os.path.join(sys.argv[1], "src", "NativeUtils")
    inc_dir = os.path.join(sys.argv[1], "include", "NativeUtils")
    cs = cases()
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(drv, "w") as f:
            f.write(DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-include", "cmath", "-I", inc_dir, drv, os.path.join(src_dir, "colorcorrection.cpp"),
                               "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.int32(len(cs)).tobytes())
            for s, d in cs:
                f.write(np.int32(len(s)).tobytes() + s.tobytes() + d.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    rec = 9 * 8 + 256 * 3
    assert len(raw) == rec * len(cs)
    arrays = {}
    for k, (s, d) in enumerate(cs):
        r = raw[k * rec:(k + 1) * rec]
        arrays[f"src_{k}"], arrays[f"dst_{k}"] = s, d
        arrays[f"xform_{k}"] = np.frombuffer(r[:72], dtype="<f8").copy()
        arrays[f"applied_{k}"] = np.frombuffer(r[72:], dtype=np.uint8).reshape(256, 3).copy()
    arrays["n_cases"] = np.int32(len(cs))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(cs)} cases")


if __name__ == "__main__":
    main()
