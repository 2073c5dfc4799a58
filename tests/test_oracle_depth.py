"""The CPU oracle's depth -> cloud path against an independent numpy-float32 op-by-op restatement of
createVertices (src/NativeUtils/depthprocessing.cpp:122-187) and against committed digests.

Status: pinned.  The reference's own exports, compiled with stand-ins (tests/golden/make_export_golden.py), are recorded in
tests/golden/export_ref.npz / export_ref_digests.json; tests/test_export_pin.py holds the C oracle and numpy_create_vertices
(tests/depth_ref.py) to them.  Here: the two independently written restatements (C and numpy) agree bit for bit, and the C one does not drift (sha256 of
its output on seeded inputs, tests/golden/digests.json)."""
import json
import os

import numpy as np
import pytest

from livescan3d_amd import synth
from tests.depth_ref import numpy_create_vertices


def _frames(rig):
    d = rig.depth_maps.view(np.uint16)
    pos_d, pos_c = 0, 0
    for i in range(rig.n):
        w, h = int(rig.widths[i]), int(rig.heights[i])
        yield (d[pos_d:pos_d + w * h].reshape(h, w), rig.depth_colors[pos_c:pos_c + 3 * w * h].reshape(h, w, 3),
               rig.intr[7 * i:7 * i + 7], rig.wt[12 * i:12 * i + 12])
        pos_d += w * h
        pos_c += 3 * w * h


@pytest.mark.parametrize("kind,n,w,h", [("noise", 2, 64, 48), ("scene", 3, 128, 96), ("noise", 1, 512, 424), ("scene", 2, 512, 424)])
def test_c_oracle_equals_numpy_restatement(orc, kind, n, w, h):
    rig = synth.make_rig(kind, n, w, h, seed=9)
    got, counts = orc.generate_mesh_vertices(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    want = np.concatenate([numpy_create_vertices(d, c, i, t, rig.bounds) for d, c, i, t in _frames(rig)])
    assert len(want) > 0
    assert got.tobytes() == want.tobytes()
    assert counts.sum() == len(got)
    # the single-sensor export agrees with the merged call's slices (depthprocessing.cpp:1631-1657)
    e = np.concatenate([[0], np.cumsum(counts)])
    for i in range(n):
        one = orc.generate_vertices_from_depth_map(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, i)
        assert one.tobytes() == got[e[i]:e[i + 1]].tobytes()
    # the thread-per-sensor fan-out changes nothing
    got4, _ = orc.generate_mesh_vertices(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, n_threads=4)
    assert got4.tobytes() == got.tobytes()


def test_maps_and_raster_order(orc):
    d, c = synth.noise_frame(4, 0, 0, 40, 30)
    intr = synth.kinect_intrinsics(40, 30)
    wt = synth.pack_pose(*synth.ring_pose(0, 1))
    v, v2p, p2v = orc.create_vertices(d, c, intr, wt, [-0.3, -0.3, -1.5, 0.3, 0.3, 1.5], want_maps=True)
    assert len(v) > 10 and (np.diff(v2p) > 0).all()                       # raster order (depthprocessing.cpp:166-175)
    assert (p2v[v2p] == np.arange(len(v))).all() and (p2v >= -1).all() and (p2v == -1).sum() == 40 * 30 - len(v)
    assert (d.ravel()[v2p] != 0).all()


def test_edge_cases(orc):
    w, h = 16, 8
    intr = synth.kinect_intrinsics(w, h)
    wt = synth.pack_pose(*synth.ring_pose(0, 1))
    rgb = synth.noise_frame(1, 0, 0, w, h)[1]
    zero = np.zeros((h, w), np.uint16)
    assert len(orc.create_vertices(zero, rgb, intr, wt, synth.DEFAULT_BOUNDS)) == 0
    full = np.full((h, w), 2000, np.uint16)
    v = orc.create_vertices(full, rgb, intr, wt, synth.DEFAULT_BOUNDS)
    assert len(v) == w * h and (v["A"] == 255).all()
    # inclusive bounds: the box that is exactly the min/max of the cloud keeps everything
    b = [v["X"].min(), v["Y"].min(), v["Z"].min(), v["X"].max(), v["Y"].max(), v["Z"].max()]
    assert len(orc.create_vertices(full, rgb, intr, wt, b)) == w * h
    # NaN pose: every comparison is false, the vertex is kept (depthprocessing.cpp:162)
    wt_nan = wt.copy()
    wt_nan[1] = np.nan
    vn = orc.create_vertices(full, rgb, intr, wt_nan, synth.DEFAULT_BOUNDS)
    assert len(vn) == w * h and np.isnan(vn["Y"]).any()
    # no sensors at all
    e, counts = orc.generate_mesh_vertices(np.zeros(0, np.uint8), np.zeros(0, np.uint8), [], [], [], [], synth.DEFAULT_BOUNDS)
    assert len(e) == 0


DIGEST_CASES = [("noise", 8, 512, 424, 3), ("scene", 8, 512, 424, 3), ("noise", 2, 1024, 1024, 3)]


def test_oracle_output_digests(orc):
    """Regression pin of the oracle on BASELINE-sized rigs; regenerate with LSN_WRITE_DIGESTS=1."""
    path = os.path.join(os.path.dirname(__file__), "golden", "digests.json")
    have = json.load(open(path)) if os.path.exists(path) else {}
    fresh = {}
    for (kind, n, w, h, seed) in DIGEST_CASES:
        rig = synth.make_rig(kind, n, w, h, seed=seed)
        v, counts = orc.generate_mesh_vertices(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, n_threads=4)
        fresh[f"{kind}-{n}x{w}x{h}-seed{seed}"] = {
            "inputs": synth.digest(np.concatenate([rig.depth_maps, rig.depth_colors])), "n_vertices": int(len(v)),
            "counts": [int(c) for c in counts], "vertices": synth.digest(v)}
    if os.environ.get("LSN_WRITE_DIGESTS"):
        json.dump(fresh, open(path, "w"), indent=1, sort_keys=True)
        have = fresh
    assert have, "tests/golden/digests.json missing: run once with LSN_WRITE_DIGESTS=1"
    assert fresh == have
