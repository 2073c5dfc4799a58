#!/usr/bin/env python3
"""Regenerates tests/golden/overlay_merge_ref.npz: the reference's own drawTriangle, morphologyErode and pointProjection
(src/NativeUtils/depthprocessing.cpp:592-706, 735-747, 903-930, with RotatePoint :109-120) run on fixed inputs.

    python tests/golden/make_merge_golden.py <LiveScan3D checkout>

depthprocessing.cpp as a whole needs <windows.h>, so those functions are cut out of it by name into a temporary directory, behind
stand-in declarations written here (Point3f, WorldTranformation with inv(), IntrinsicCameraParameters, min / max), compiled with g++
on x86-64 together with a small driver, and run; nothing of the reference is kept -- only the results.

Cases:
  * draw_<k>: sequences of triangles {x1,y1,d1, x2,y2,d2, x3,y3,d3} with their unsigned short tags, drawn in order into one zeroed
    map (the depth map and the tag map after the sequence): random triangles, degenerate and edge-on ones, val near 0 and near
    65535 (where x64's float -> unsigned short wraps), and zero-val overdraw;
  * erode_<k>: masks before / after one morphologyErode (random densities, set border pixels, tiny sizes);
  * proj: points projected with inverted random poses and intrinsics (behind the camera, far away, NaN-producing z = 0)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "overlay_merge_ref.npz")
W, H = 48, 40

PRELUDE = r"""
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace std;
struct Point3f { float X, Y, Z; };
struct WorldTranformation {   // depthprocessing.h: t, then R row by row; inv() = (R^T, -t)
    std::vector<float> t;
    std::vector<std::vector<float>> R;
    WorldTranformation(const float *p) : t(p, p + 3), R(3, std::vector<float>(3)) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i][j] = p[3 + 3 * i + j];
    }
    void inv() {
        std::vector<std::vector<float>> Rt(3, std::vector<float>(3));
        for (int i = 0; i < 3; i++) { t[i] = -t[i]; for (int j = 0; j < 3; j++) Rt[i][j] = R[j][i]; }
        R = Rt;
    }
};
struct IntrinsicCameraParameters {
    float cx, cy, fx, fy, r2, r4, r6;
    IntrinsicCameraParameters(const float *p) : cx(p[0]), cy(p[1]), fx(p[2]), fy(p[3]), r2(p[4]), r4(p[5]), r6(p[6]) {}
};
"""

DRIVER = r"""
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) exit(2); }
int main(int argc, char **argv)
{
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int n_draw, n_erode, n_proj;
    rd(&n_draw, 4, in);
    for (int c = 0; c < n_draw; c++) {
        int w, h, m;
        rd(&w, 4, in); rd(&h, 4, in); rd(&m, 4, in);
        std::vector<int> t(9 * (size_t)m);
        std::vector<unsigned short> tags(m);
        if (m) { rd(t.data(), 36 * (size_t)m, in); rd(tags.data(), 2 * (size_t)m, in); }
        std::vector<unsigned short> depth((size_t)w * h, 0), tag2((size_t)w * h, 0);
        std::vector<float> tag1((size_t)w * h, 0.0f);
        for (int k = 0; k < m; k++) {
            const int *q = &t[9 * (size_t)k];
            drawTriangle(q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], depth.data(), w, h, tag1.data(), 0.5f, tag2.data(), tags[k]);
        }
        fwrite(depth.data(), 2, depth.size(), out);
        fwrite(tag2.data(), 2, tag2.size(), out);
    }
    rd(&n_erode, 4, in);
    for (int c = 0; c < n_erode; c++) {
        int w, h;
        rd(&w, 4, in); rd(&h, 4, in);
        std::vector<unsigned char> m((size_t)w * h);
        rd(m.data(), m.size(), in);
        morphologyErode(m, w, h);
        fwrite(m.data(), 1, m.size(), out);
    }
    rd(&n_proj, 4, in);
    for (int c = 0; c < n_proj; c++) {
        float p[3], wt[12], ip[7];
        rd(p, 12, in); rd(wt, 48, in); rd(ip, 28, in);
        Point3f pt = {p[0], p[1], p[2]};
        WorldTranformation T(wt);
        T.inv();
        IntrinsicCameraParameters I(ip);
        int x, y; unsigned short d;
        pointProjection(pt, x, y, d, T, I);
        int r[3] = {x, y, (int)d};
        fwrite(r, 4, 3, out);
    }
    fclose(out);
    return 0;
}
"""

FUNCTIONS = [r"void RotatePoint\(", r"inline int iround\(", r"void drawTriangle\(", r"void pointProjection\(", r"void morphologyErode\("]


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


def draw_cases():
    rng = np.random.default_rng(20261015)
    cases = []

    def tri(x, y, d):
        return [x[0], y[0], d[0], x[1], y[1], d[1], x[2], y[2], d[2]]

    def rand_tris(m, dlo, dhi, span):
        out = []
        for _ in range(m):
            cx, cy = rng.integers(1, W - 1), rng.integers(1, H - 1)
            x = np.clip(cx + rng.integers(-span, span + 1, 3), 1, W - 1)
            y = np.clip(cy + rng.integers(-span, span + 1, 3), 1, H - 1)
            out.append(tri(x, y, rng.integers(dlo, dhi, 3)))
        return out

    cases.append(rand_tris(300, 500, 4000, 3))                              # small random triangles, both orientations
    cases.append(rand_tris(60, 500, 4000, 20))                              # large ones, heavy overdraw
    cases.append([tri([5, 5, 5], [5, 10, 20], [1000] * 3), tri([3, 9, 15], [7, 7, 7], [900, 950, 1000]),   # degenerate: den == 0
                  tri([4, 4, 4], [4, 4, 4], [800] * 3), tri([10, 20, 30], [10, 15, 20], [700, 800, 900])])
    cases.append([tri([2, 30, 30], [2, 2, 3], [1500, 1600, 1700]), tri([2, 3, 3], [2, 2, 35], [1200, 1300, 1400]),  # edge-on slivers
                  tri([1, 46, 1], [1, 38, 2], [2000, 2100, 2200])])
    near0 = []
    for _ in range(80):                                                    # val near 0: tiny depths, interpolation to 0
        near0 += rand_tris(1, 1, 3, 4)
    cases.append(near0)
    near_max = rand_tris(150, 65530, 65536, 5)                              # val near 65535: a hair above wraps to 0 on x64
    near_max += [tri([1, 40, 20], [1, 5, 38], [65535, 65535, 65535]), tri([1, 40, 20], [1, 5, 38], [65535, 1, 65535])]
    cases.append(near_max)
    zero = []                                                              # zero-val overdraw: a val-0 write, then anything writes
    for k in range(40):
        zero += rand_tris(1, 1, 2, 6) if k % 3 == 0 else rand_tris(1, 300, 900, 6)
    cases.append(zero)
    cases.append(rand_tris(400, 1, 65536, 4))                               # everything mixed
    # one shared tag per triangle, u16 (the confidence averages are 0..20; the full range is pinned too)
    return [(np.array(c, dtype=np.int32).reshape(-1, 9), rng.integers(0, 65536, len(c)).astype(np.uint16)) for c in cases]


def erode_cases():
    rng = np.random.default_rng(7)
    out = []
    for (w, h), p in (((48, 40), 0.5), ((48, 40), 0.85), ((48, 40), 0.97), ((3, 3), 1.0), ((2, 5), 1.0), ((17, 4), 0.9), ((1, 1), 1.0)):
        out.append(((rng.random((h, w)) < p) * 255).astype(np.uint8))
    m = np.zeros((40, 48), np.uint8)
    m[:, :] = 255
    m[20, 30] = 0                                                          # one hole in a full mask: border stays set
    out.append(m)
    return out


def proj_cases():
    rng = np.random.default_rng(11)
    out = []
    for k in range(400):
        ang = rng.uniform(-np.pi, np.pi, 3)
        cz, sz, cy_, sy = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1])
        R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]])
        t = rng.uniform(-3, 3, 3)
        wt = np.concatenate([t, R.ravel()]).astype(np.float32)
        ip = np.array([rng.uniform(200, 300), rng.uniform(180, 240), rng.uniform(300, 400), rng.uniform(300, 400), 0, 0, 0], np.float32)
        p = rng.uniform(-5, 5, 3).astype(np.float32)
        if k % 50 == 0:
            p = (R @ t).astype(np.float32)                                 # z = 0 in the camera: inf / NaN
        if k % 50 == 1:
            p = (p * 1e5).astype(np.float32)                               # far away: d clamps to 65535
        out.append((p, wt, ip))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src = open(os.path.join(sys.argv[1], "src", "NativeUtils", "depthprocessing.cpp"), encoding="utf-8", errors="replace").read()
    dc, ec, pc = draw_cases(), erode_cases(), proj_cases()
    with tempfile.TemporaryDirectory() as tmp:
        drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(drv, "w") as f:
            f.write(PRELUDE + "".join(cut(src, p) for p in FUNCTIONS) + DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", drv, "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.int32(len(dc)).tobytes())
            for t, tags in dc:
                f.write(np.int32([W, H, len(t)]).tobytes() + t.tobytes() + tags.tobytes())
            f.write(np.int32(len(ec)).tobytes())
            for m in ec:
                f.write(np.int32([m.shape[1], m.shape[0]]).tobytes() + m.tobytes())
            f.write(np.int32(len(pc)).tobytes())
            for p, wt, ip in pc:
                f.write(p.tobytes() + wt.tobytes() + ip.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    arrays, pos = {}, 0
    for k, (t, tags) in enumerate(dc):
        n = W * H * 2
        arrays[f"draw_tris_{k}"], arrays[f"draw_tags_{k}"] = t, tags
        arrays[f"draw_depth_{k}"] = np.frombuffer(raw[pos:pos + n], "<u2").reshape(H, W).copy()
        arrays[f"draw_tag_{k}"] = np.frombuffer(raw[pos + n:pos + 2 * n], "<u2").reshape(H, W).copy()
        pos += 2 * n
    for k, m in enumerate(ec):
        arrays[f"erode_in_{k}"] = m
        arrays[f"erode_out_{k}"] = np.frombuffer(raw[pos:pos + m.size], np.uint8).reshape(m.shape).copy()
        pos += m.size
    arrays["proj_p"] = np.stack([p for p, _, _ in pc])
    arrays["proj_wt"] = np.stack([wt for _, wt, _ in pc])
    arrays["proj_ip"] = np.stack([ip for _, _, ip in pc])
    arrays["proj_out"] = np.frombuffer(raw[pos:pos + 12 * len(pc)], "<i4").reshape(-1, 3).copy()
    pos += 12 * len(pc)
    assert pos == len(raw)
    arrays["n_draw"], arrays["n_erode"], arrays["size"] = np.int32(len(dc)), np.int32(len(ec)), np.int32([W, H])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(dc)} draw, {len(ec)} erode, {len(pc)} projection cases")


if __name__ == "__main__":
    main()
