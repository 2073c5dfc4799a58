#!/usr/bin/env python3
"""Regenerates tests/golden/outlier_filter_ref.npz: the reference's own KNNeighbors and filter() (src/LiveScanClient/filter.cpp:19-81)
over its PointCloud / kdTree (include/LiveScanClient/filter.h) and its nanoflann (include/nanoflann.h, 0x119), run on fixed clouds.

    python tests/golden/make_outlier_golden.py <LiveScan3D checkout>

filter.h includes utils.h, which pulls in stdafx.h / <windows.h>; so filter.h is read into a temporary directory beside a stand-in utils.h
written here (Point3f, RGB), the two functions are cut out of filter.cpp by name, and the whole is compiled with g++ on x86-64
(-O2 -ffp-contract=off, like the reference's /fp:precise; the `#pragma omp` is inert without -fopenmp) together with a small driver, and
run; nothing of the reference is kept -- only the results.

Clouds: sensor blocks of the scene, ring and wall rigs (the oracle's createVertices, what generateVerticesFromDepthMap returns), Gaussian
clusters with sparse far outliers, a cloud with 20 % duplicated points, a lattice full of exact ties.  Settings per cloud: k in
{1, 2, 10, n, n + 1} with a maxDist whose float square is a recorded kDistance, one float step either side, 0.01 and 0.05, a maxDist whose
square overflows to inf, the one whose square is the largest finite float; and k = 0, k = -1, maxDist = 0, maxDist = -1, maxDist = NaN.
Recorded: kDistance of every point per (cloud, k >= 1); per case changedVerticesMap (its values for keys 0..n-1, empty after the
early return; key -1 maps to -1 in every case), which is the keep mask and the new indices; and -- for the cases
at the recorded kDistance -- the filtered vertices and colours."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "outlier_filter_ref.npz")

UTILS_STANDIN = r"""
#pragma once
#include <cmath>
struct Point3f { float X, Y, Z; };
typedef struct RGB { unsigned char rgbBlue, rgbGreen, rgbRed, rgbReserved; } RGB;
"""

DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
static void rd(void *p, size_t n, FILE *f) { if (fread(p, 1, n, f) != n) exit(2); }
int main(int argc, char **argv)
{
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int n_cases;
    rd(&n_cases, 4, in);
    for (int c = 0; c < n_cases; c++) {
        int n, k;
        float maxDist;
        rd(&n, 4, in); rd(&k, 4, in); rd(&maxDist, 4, in);
        std::vector<Point3f> v(n);
        std::vector<RGB> col(n);
        rd(v.data(), 12 * (size_t)n, in);
        rd(col.data(), 4 * (size_t)n, in);
        if (k >= 1) {   // KNNeighbors' kDistance, as filter() computes it (filter.cpp:43-49)
            PointCloud cloud;
            cloud.pts = v;
            kdTree tree(3, cloud);
            tree.buildIndex();
            std::vector<KNNeighborsResult> knn = KNNeighbors(cloud, tree, k);
            for (int i = 0; i < n; i++) fwrite(&knn[i].kDistance, 4, 1, out);
        }
        std::unordered_map<int, int> m = filter(v, col, k, maxDist);
        int nv = (int)v.size(), nm = (int)m.size();
        fwrite(&nv, 4, 1, out);
        fwrite(v.data(), 12, (size_t)nv, out);
        fwrite(col.data(), 4, (size_t)nv, out);
        std::vector<std::pair<int, int>> e(m.begin(), m.end());
        std::sort(e.begin(), e.end());
        fwrite(&nm, 4, 1, out);
        for (auto &kv : e) { fwrite(&kv.first, 4, 1, out); fwrite(&kv.second, 4, 1, out); }
    }
    fclose(out);
    return 0;
}
"""

FUNCTIONS = [r"vector<KNNeighborsResult> KNNeighbors\(", r"unordered_map<int, int> filter\("]


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


def clouds():
    """name -> (vertices (n, 3) float32, colours (n, 3) uint8)."""
    from livescan3d_amd import synth
    from oracle import orc
    from tests import color_cases, merge_cases
    orc.build()
    out = {}
    rigs = {"scene": synth.make_rig("scene", 2, 48, 40, seed=3), "ring": color_cases.ring(2, sizes=[(48, 40)] * 2, of=8),
            "wall": merge_cases.wall(2, 40, 32)}
    for name, rig in rigs.items():
        dm, p = rig.depth_maps.view("<u2"), 0
        for i in range(rig.n):
            w, h = int(rig.widths[i]), int(rig.heights[i])
            v = orc.create_vertices(dm[p:p + w * h].reshape(h, w), rig.depth_colors[3 * p:3 * (p + w * h)].reshape(h, w, 3),
                                    rig.intr[7 * i:7 * i + 7], rig.wt[12 * i:12 * i + 12], rig.bounds)
            p += w * h
            if i == 0:   # one block per rig
                out[f"{name}_block"] = (np.stack([v["X"], v["Y"], v["Z"]], 1).astype(np.float32), np.stack([v["R"], v["G"], v["B"]], 1))
    rng = np.random.default_rng(20261016)
    g = np.concatenate([rng.normal(0, 0.05, (500, 3)), rng.normal(1, 0.02, (250, 3)), rng.uniform(-3, 3, (15, 3))]).astype(np.float32)
    out["gauss_outliers"] = (g, rng.integers(0, 256, (len(g), 3)).astype(np.uint8))
    base = rng.normal(0, 0.03, (480, 3)).astype(np.float32)
    dup = np.concatenate([base, base[rng.integers(0, len(base), 120)]])
    out["duplicates"] = (dup, rng.integers(0, 256, (len(dup), 3)).astype(np.uint8))
    lat = (np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(6), indexing="ij"), -1).reshape(-1, 3) * 0.01).astype(np.float32)
    out["lattice"] = (lat, rng.integers(0, 256, (len(lat), 3)).astype(np.uint8))
    return out


def largest_finite_root():
    """The float m whose float square m * m is the largest finite float."""
    m = np.float32(np.sqrt(np.float64(np.finfo(np.float32).max)))
    with np.errstate(over="ignore"):
        while np.isinf(m * m):
            m = np.nextafter(m, np.float32(0))
        while not np.isinf(np.nextafter(m, np.float32(np.inf)) * np.nextafter(m, np.float32(np.inf))):
            m = np.nextafter(m, np.float32(np.inf))
    return m


def exact_root(finite):
    """A float m whose float square m * m IS one of the recorded kDistance values (from the median up), or None."""
    for v in np.concatenate([finite[len(finite) // 2:], finite[:len(finite) // 2][::-1]]):
        m = np.float32(np.sqrt(np.float64(v)))
        for _ in range(4):
            for c in (m, np.nextafter(m, np.float32(0)), np.nextafter(m, np.float32(np.inf))):
                if np.float32(c * c) == v and v > 0:
                    return np.float32(c)
            m = np.nextafter(m, np.float32(0))
    return None


def settings(pts, kd_of):
    """(k, maxDist, keep_arrays) per case for one cloud; kd_of(k) gives a recorded kDistance array (numpy brute force, used only to
    place the boundary thresholds -- the fixture records the reference's own values)."""
    n = len(pts)
    big = largest_finite_root()
    out = []
    for k in (1, 2, 10, n, n + 1):
        kd = kd_of(k)
        finite = np.sort(kd[kd < np.finfo(np.float32).max])
        ds = []
        b = exact_root(finite)
        if b is not None:
            ds += [(b, True), (np.nextafter(b, np.float32(0)), False), (np.nextafter(b, np.float32(1e30)), False)]
        ds += [(np.float32(0.01), False), (np.float32(0.05), False), (np.float32(1e20), False), (big, False)]
        out += [(k, d, keep) for d, keep in ds]
    out += [(0, np.float32(0.05), False), (-1, np.float32(0.05), False), (10, np.float32(0.0), False), (10, np.float32(-1.0), False),
            (10, np.float32(np.nan), False)]
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    from tests import outlier_ref
    ref = sys.argv[1]
    src = open(os.path.join(ref, "src", "LiveScanClient", "filter.cpp"), encoding="utf-8", errors="replace").read()
    cl = clouds()
    cases = []
    for name, (pts, rgb) in cl.items():
        for k, d, keep in settings(pts, lambda k: outlier_ref.k_distance(pts, k)):
            cases.append((name, int(k), np.float32(d), keep))
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(os.path.join(ref, "include", "LiveScanClient", "filter.h"), os.path.join(tmp, "filter.h"))
        with open(os.path.join(tmp, "utils.h"), "w") as f:
            f.write(UTILS_STANDIN)
        drv, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        with open(drv, "w") as f:
            f.write('#include "filter.h"\n#include <unordered_map>\nusing namespace std;\n' + "".join(cut(src, p) for p in FUNCTIONS) + DRIVER)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I", tmp, "-I", os.path.join(ref, "include"), drv,
                               "-o", exe])
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.int32(len(cases)).tobytes())
            for name, k, d, _ in cases:
                pts, rgb = cl[name]
                rgba = np.zeros((len(pts), 4), np.uint8)
                rgba[:, 0], rgba[:, 1], rgba[:, 2] = rgb[:, 2], rgb[:, 1], rgb[:, 0]   # RGB = {rgbBlue, rgbGreen, rgbRed, rgbReserved}
                f.write(np.int32([len(pts), k]).tobytes() + d.tobytes() + pts.tobytes() + rgba.tobytes())
        subprocess.check_call([exe, fin, fout])
        raw = open(fout, "rb").read()
    arrays, pos = {}, 0
    names = list(cl)
    for name in names:
        arrays[f"cloud_{name}"], arrays[f"colors_{name}"] = cl[name]
    arrays["cloud_names"] = np.array(names)
    case_cloud, case_k, case_d = [], [], []
    for c, (name, k, d, keep_arrays) in enumerate(cases):
        n = len(cl[name][0])
        if k >= 1:   # kDistance depends on the cloud and k alone: kept once per pair (every case's run is checked to agree)
            kd = np.frombuffer(raw[pos:pos + 4 * n], "<f4").copy()
            key = f"kdist_{name}_{k}"
            assert key not in arrays or arrays[key].tobytes() == kd.tobytes(), key
            arrays[key] = kd
            pos += 4 * n
        nv = int(np.frombuffer(raw[pos:pos + 4], "<i4")[0])
        pos += 4
        v = np.frombuffer(raw[pos:pos + 12 * nv], "<f4").reshape(-1, 3).copy()
        pos += 12 * nv
        col = np.frombuffer(raw[pos:pos + 4 * nv], np.uint8).reshape(-1, 4)[:, [2, 1, 0]].copy()
        pos += 4 * nv
        nm = int(np.frombuffer(raw[pos:pos + 4], "<i4")[0])
        pos += 4
        kv = np.frombuffer(raw[pos:pos + 8 * nm], "<i4").reshape(-1, 2).copy()
        pos += 8 * nm
        # changedVerticesMap: {-1: -1} alone (the early return) or {-1: -1, 0: .., .., n-1: ..}; kept as its values for keys 0..n-1
        assert kv[0].tolist() == [-1, -1] and (nm == 1 or np.array_equal(kv[1:, 0], np.arange(n))), (name, k, d)
        arrays[f"changed_{c}"] = kv[1:, 1].astype(np.int32)
        if keep_arrays:
            arrays[f"filtered_vertices_{c}"], arrays[f"filtered_colors_{c}"] = v, col
        case_cloud.append(names.index(name))
        case_k.append(k)
        case_d.append(d)
    assert pos == len(raw)
    arrays["case_cloud"], arrays["case_k"], arrays["case_max_dist"] = np.int32(case_cloud), np.int32(case_k), np.float32(case_d)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}: {len(names)} clouds, {len(cases)} cases, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
