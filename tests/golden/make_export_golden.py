#!/usr/bin/env python3
"""Regenerates tests/golden/export_ref.npz and tests/golden/export_ref_digests.json: the reference's own exports
(generateMeshFromDepthMaps, generateVerticesFromDepthMap, depthMapAndColorSetRadialCorrection of src/NativeUtils/depthprocessing.cpp)
run on the inputs of tests/export_cases.py.

    python tests/golden/make_export_golden.py <LiveScan3D checkout> [output directory]

depthprocessing.cpp is copied into a temporary directory and compiled there with g++ on x86-64 (-O2 -ffp-contract=off: every float
operation rounds on its own, as MSVC's /fp:precise does), together with meshGenerator.cpp and colorcorrection.cpp read where they lie
and a small driver written here.  Nothing of the reference is kept -- only the results.

Stand-ins, written by this script into the temporary directory ahead of the reference's include paths:
  * simpletimer.h  -- start / stop / printLapTimeAndRestart do nothing (they only read the clock and print);
  * simpleimage.h  -- create() allocates, data_ptr points at the pixels, writeToFile() does nothing (the real one needs <windows.h>);
  * pgm.h          -- writePGM does nothing (debug images only);
  * thread         -- std::thread runs its function at once, in the constructing thread, and join() does nothing.  g++ rejects the
                      MSVC-only thread(f, ..., intrinsic_params[i]) that binds a non-const reference; the shim passes it on as it is.
Two text edits of the copy:
  * "#define LOAD_FRAMES_INFORMATION" is dropped: as shipped, generateMeshFromDepthMaps ignores its arguments and loads
    frames_info_3_na_gorze.bin;
  * writeDepthImage returns at once (it only writes debug images).
None of them changes a result: every per-sensor thread writes only its own VerticesWithDepthColorMaps (or its own frame, or its own
partial triangle list, which the caller concatenates in thread order), so running the threads in order computes what running them side
by side does, and the stubs only write debug files or read the time.

Left out, and kept on the restatements (tests/color_ref.py, tests/merge_ref.py): the two cases DESIGN.md section 2 defines rather than
copies -- a crop box through the overlap of colour transfer, where the reference reads colors1[-3], and sensors of different sizes under
the overlay merge.

Outputs: export_ref.npz holds tests/export_cases.SMALL with their inputs and full outputs (vertex bytes, per-sensor counts, triangles,
corrected depth and colour maps); export_ref_digests.json holds tests/export_cases.large_cases() as sha256 of the inputs and of every
output, with the vertex and triangle counts."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import export_cases  # noqa: E402

STUBS = {
    "simpletimer.h": """#pragma once
struct SimpleTimer {
    void start() {}
    void stop() {}
    int getMilliseconds() { return 0; }
    void printLapTimeAndRestart(const char *) {}
};
""",
    "simpleimage.h": """#pragma once
#include <vector>
struct SimpleImage {
    std::vector<unsigned char> pixels;
    unsigned char *data_ptr = nullptr;
    void create(int width, int height, int bytes_per_pixel, unsigned char *) {
        pixels.assign((size_t)width * height * bytes_per_pixel, 0);
        data_ptr = pixels.data();
    }
    int writeToFile(const char *) { return 0; }
};
""",
    "pgm.h": """#pragma once
template <class T> inline bool writePGM(const char *, int, int, T *) { return true; }
template <class T> inline bool writePGM(const char *, int, int, T *, unsigned char *) { return true; }
""",
    "thread": """#pragma once
#include <functional>
#include <utility>
namespace std {
class thread {
public:
    template <class F, class... A> explicit thread(F &&f, A &&... a) { f(a...); }
    thread(thread &&) = default;
    thread &operator=(thread &&) = default;
    void join() {}
};
}
""",
}

DRIVER = r"""
#include "depthprocessing.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
static FILE *in, *out;
static void rd(void *p, size_t n) { if (n && fread(p, 1, n, in) != n) exit(2); }
static void wr(const void *p, size_t n) { if (n) fwrite(p, 1, n, out); }
int main(int argc, char **argv)
{
    in = fopen(argv[1], "rb"); out = fopen(argv[2], "wb");
    if (!in || !out) return 1;
    int op;
    while (fread(&op, 4, 1, in) == 1) {
        int n, ct, tri, index;
        rd(&n, 4); rd(&ct, 4); rd(&tri, 4); rd(&index, 4);
        std::vector<int> w(n + 1), h(n + 1);
        rd(w.data(), 4 * (size_t)n); rd(h.data(), 4 * (size_t)n);
        size_t px = 0;
        for (int i = 0; i < n; i++) px += (size_t)w[i] * h[i];
        std::vector<unsigned char> depth(2 * px + 1), colors(3 * px + 1);
        std::vector<float> intr(7 * (size_t)n + 1), wt(12 * (size_t)n + 1), b(6);
        rd(depth.data(), 2 * px); rd(colors.data(), 3 * px); rd(intr.data(), 28 * (size_t)n); rd(wt.data(), 48 * (size_t)n); rd(b.data(), 24);
        if (op == 0) {          // depthMapAndColorSetRadialCorrection, in place
            depthMapAndColorSetRadialCorrection(n, depth.data(), colors.data(), w.data(), h.data(), intr.data());
            wr(depth.data(), 2 * px); wr(colors.data(), 3 * px);
            continue;
        }
        Mesh m = {0, nullptr, 0, nullptr};
        if (op == 1)
            generateMeshFromDepthMaps(n, depth.data(), colors.data(), w.data(), h.data(), intr.data(), wt.data(), &m, ct != 0,
                                      b[0], b[1], b[2], b[3], b[4], b[5], tri != 0);
        else
            generateVerticesFromDepthMap(depth.data(), colors.data(), w.data(), h.data(), intr.data(), wt.data(), &m,
                                         b[0], b[1], b[2], b[3], b[4], b[5], index);
        wr(&m.nVertices, 4); wr(&m.nTriangles, 4);
        wr(m.vertices, 16 * (size_t)m.nVertices); wr(m.triangles, 12 * (size_t)m.nTriangles);
        deleteMesh(&m);
    }
    fclose(out);
    return 0;
}
"""

OP_RADIAL, OP_MESH, OP_VERTS = 0, 1, 2


def build(ref, tmp):
    nu = os.path.join(ref, "src", "NativeUtils")
    src = open(os.path.join(nu, "depthprocessing.cpp"), encoding="utf-8", errors="replace").read()
    src, k = re.subn(r"^#define LOAD_FRAMES_INFORMATION\s*$", "", src, flags=re.M)
    assert k == 1, "LOAD_FRAMES_INFORMATION"
    src, k = re.subn(r"(void writeDepthImage\([^)]*\)\s*\{)", r"\1 return;", src)
    assert k == 1, "writeDepthImage"
    with open(os.path.join(tmp, "depthprocessing.cpp"), "w") as f:
        f.write(src)
    for name, text in STUBS.items():
        with open(os.path.join(tmp, name), "w") as f:
            f.write(text)
    with open(os.path.join(tmp, "driver.cpp"), "w") as f:
        f.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    inc = ["-I", tmp, "-I", os.path.join(ref, "include", "NativeUtils"), "-I", os.path.join(ref, "include")]
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-w", "-pthread", *inc, "-D__int64=long long",
                           "-D__declspec(x)=", "-D__stdcall=", "-DDEPTH_PROCESSING_DLL_EXPORTS", "-include", "cstring", "-include", "cmath",
                           os.path.join(tmp, "depthprocessing.cpp"), os.path.join(nu, "meshGenerator.cpp"),
                           os.path.join(nu, "colorcorrection.cpp"), os.path.join(tmp, "driver.cpp"), "-o", exe])
    return exe


def call(exe, tmp, calls):
    """calls: [(op, rig, ct, tri, index)] -> per call (depth u8, colours u8) for OP_RADIAL, (vertex bytes u8, triangles int32 (m, 3))
    otherwise."""
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        for op, r, ct, tri, index in calls:
            f.write(np.int32([op, r.n, ct, tri, index]).tobytes() + r.widths.tobytes() + r.heights.tobytes())
            f.write(r.depth_maps.tobytes() + r.depth_colors.tobytes() + r.intr.tobytes() + r.wt.tobytes() + r.bounds.tobytes())
    subprocess.check_call([exe, fin, fout])
    raw, pos, res = open(fout, "rb").read(), 0, []
    for op, r, _, _, _ in calls:
        if op == OP_RADIAL:
            px = int(np.sum(r.widths.astype(np.int64) * r.heights))
            res.append((np.frombuffer(raw, np.uint8, 2 * px, pos).copy(), np.frombuffer(raw, np.uint8, 3 * px, pos + 2 * px).copy()))
            pos += 5 * px
        else:
            nv, nt = np.frombuffer(raw, "<i4", 2, pos)
            pos += 8
            v = np.frombuffer(raw, np.uint8, 16 * nv, pos).copy()
            t = np.frombuffer(raw, "<i4", 3 * nt, pos + 16 * nv).reshape(-1, 3).copy()
            pos += 16 * nv + 12 * nt
            res.append((v, t))
    assert pos == len(raw)
    return res


def run_cases(exe, tmp, cases):
    """-> {name: {"radial_depth", "radial_colors", "counts", "v<bcolor_transfer>", "t<bgenerate_triangles>"}} from the reference."""
    results = {}
    for name, kind, rig, flags in cases:
        out = {}
        if kind in ("radial", "radial_mesh"):
            out["radial_depth"], out["radial_colors"] = call(exe, tmp, [(OP_RADIAL, rig, 0, 0, 0)])[0]
            rig = export_cases.corrected_rig(rig, out["radial_depth"], out["radial_colors"])
        if kind in ("mesh", "radial_mesh"):
            res = call(exe, tmp, [(OP_MESH, rig, ct, tri, 0) for ct, tri in flags] + [(OP_VERTS, rig, 0, 0, i) for i in range(rig.n)])
            for (ct, tri), (v, t) in zip(flags, res):
                # colour transfer changes colours only and the overlay merge triangles only: one cloud per bcolor_transfer and one
                # triangle list per bgenerate_triangles, whatever the other flag is
                for key, a in ((f"v{ct}", v), (f"t{tri}", t)):
                    assert key not in out or out[key].tobytes() == a.tobytes(), (name, key)
                    out[key] = a
            per = res[len(flags):]
            out["counts"] = np.int32([len(v) // 16 for v, _ in per])
            # generateVerticesFromDepthMap for every index, concatenated, is the (false, false) cloud
            out["vertices_by_index"] = np.concatenate([v for v, _ in per]) if per else np.zeros(0, np.uint8)
        results[name] = out
    return results


def faces_from(v, q):
    """A box {min, max} whose faces are the q and 1 - q quantiles of the reference's own coordinates (exact vertex values)."""
    xyz = np.frombuffer(v.tobytes(), np.float32).reshape(-1, 4)[:, 1:]
    k = int(q * (len(xyz) - 1))
    srt = np.sort(xyz, axis=0)
    return np.float32([srt[k, 0], srt[k, 1], srt[k, 2], srt[-1 - k, 0], srt[-1 - k, 1], srt[-1 - k, 2]])


def crop_cases(exe, tmp):
    from livescan3d_amd import synth
    out = []
    for name, rig in export_cases.crop_probe_cases():
        v = call(exe, tmp, [(OP_MESH, rig, 0, 0, 0)])[0][0]
        for q in (0.0, 0.2, 0.45):
            b = faces_from(v, q)
            out.append((f"{name}_q{int(100 * q):02d}", "mesh", synth.Rig(*zip(*export_cases.split(rig)), rig.intr, rig.wt, b), export_cases.FF))
    return out


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    outdir = sys.argv[2] if len(sys.argv) == 3 else os.path.join(ROOT, "tests", "golden")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(sys.argv[1], tmp)
        small = export_cases.SMALL + crop_cases(exe, tmp)
        res = run_cases(exe, tmp, small)
        arrays = {"cases": np.array([c[0] for c in small])}
        for name, kind, rig, flags in small:
            p = name + "/"
            arrays[p + "kind"] = np.array(kind)
            arrays[p + "flags"] = np.int32(flags).reshape(-1, 2)
            arrays[p + "widths"], arrays[p + "heights"] = rig.widths, rig.heights
            arrays[p + "depth"], arrays[p + "colors"] = rig.depth_maps.view("<u2"), rig.depth_colors
            arrays[p + "intr"], arrays[p + "wt"], arrays[p + "bounds"] = rig.intr, rig.wt, rig.bounds
            for k, a in res[name].items():
                if k != "vertices_by_index":
                    arrays[p + k] = a.view("<u2") if k == "radial_depth" else a
            if "v0" in res[name]:
                assert res[name]["vertices_by_index"].tobytes() == res[name]["v0"].tobytes(), name
        np.savez_compressed(os.path.join(outdir, "export_ref.npz"), **arrays)
        large = export_cases.large_cases()
        res = run_cases(exe, tmp, large)
        digests = {}
        for name, kind, rig, flags in large:
            r = res[name]
            e = {"kind": kind, "flags": [list(f) for f in flags], "inputs": export_cases.sha(export_cases.rig_inputs(rig))}
            for k, a in sorted(r.items()):
                if k == "vertices_by_index":
                    assert "v0" not in r or a.tobytes() == r["v0"].tobytes(), name
                    continue
                e[k] = export_cases.sha(a)
                if k.startswith("v"):
                    e["n_" + k] = len(a) // 16
                elif k.startswith("t"):
                    e["n_" + k] = len(a)
            if "counts" in r:
                e["counts"] = [int(c) for c in r["counts"]]
            digests[name] = e
        with open(os.path.join(outdir, "export_ref_digests.json"), "w") as f:
            json.dump(digests, f, indent=1, sort_keys=True)
            f.write("\n")
    print(f"wrote {outdir}: {len(small)} fixture cases, {len(large)} digest cases")


if __name__ == "__main__":
    main()
