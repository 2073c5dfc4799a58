"""The CPU reference of the overlay merge (tests/merge_ref.py) against the reference's own drawTriangle, morphologyErode and
pointProjection (tests/golden/overlay_merge_ref.npz, made by tests/golden/make_merge_golden.py), and its closed forms against plain
sequential restatements.  No GPU."""
import os

import numpy as np
import pytest

from tests import color_cases, color_ref, merge_cases, merge_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_merge_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_draw_matches_reference(golden):
    W, H = (int(v) for v in golden["size"])
    for k in range(int(golden["n_draw"])):
        tris, tags = golden[f"draw_tris_{k}"], golden[f"draw_tags_{k}"]
        d, t = merge_ref.draw(tris, tags, W, H)
        assert np.array_equal(d, golden[f"draw_depth_{k}"]), k
        assert np.array_equal(t, golden[f"draw_tag_{k}"]), k


def test_draw_sequential_matches_reference(golden):
    W, H = (int(v) for v in golden["size"])
    for k in range(int(golden["n_draw"])):
        d, t = merge_ref.draw_sequential(golden[f"draw_tris_{k}"], golden[f"draw_tags_{k}"], W, H)
        assert np.array_equal(d, golden[f"draw_depth_{k}"]), k
        assert np.array_equal(t, golden[f"draw_tag_{k}"]), k


def test_fixture_exercises_the_edge_cases(golden):
    """The fixture holds what it claims: vals at the top of the u16 range, zero-val overdraw, degenerate triangles drawing nothing."""
    W, H = (int(v) for v in golden["size"])
    top = zero_over = 0
    for k in range(int(golden["n_draw"])):
        tris = golden[f"draw_tris_{k}"]
        s = merge_ref.triangle_setup(*tris.astype(np.int64).T)
        kk, px, py, val = merge_ref.triangle_pixels(s)
        d = np.stack([s["fd"][0][kk], s["fd"][1][kk], s["fd"][2][kk]])
        top += int(((val >= 65530) & (d.min(0) > 65000)).sum())
        zero_over += int((val == 0).sum())
    assert top > 0 and zero_over > 0
    d, _ = merge_ref.draw(golden["draw_tris_2"][:1], golden["draw_tags_2"][:1], W, H)
    assert not d.any()


def test_closed_form_equals_sequential_on_random_overdraw():
    rng = np.random.default_rng(5)
    W, H = 24, 20
    for trial in range(40):
        m = int(rng.integers(1, 60))
        cx, cy = rng.integers(1, W - 1, m), rng.integers(1, H - 1, m)
        x = np.clip(cx[:, None] + rng.integers(-6, 7, (m, 3)), 1, W - 1)
        y = np.clip(cy[:, None] + rng.integers(-6, 7, (m, 3)), 1, H - 1)
        lo = 1 if trial % 2 else 300
        d = rng.integers(lo, lo + 8 if trial % 4 == 1 else 3000, (m, 3))
        tris = np.stack([x[:, 0], y[:, 0], d[:, 0], x[:, 1], y[:, 1], d[:, 1], x[:, 2], y[:, 2], d[:, 2]], axis=1)
        tags = rng.integers(0, 21, m)
        a = merge_ref.draw(tris, tags, W, H)
        b = merge_ref.draw_sequential(tris, tags, W, H)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), trial


def test_erode_matches_reference_and_loop(golden):
    for k in range(int(golden["n_erode"])):
        m = golden[f"erode_in_{k}"] != 0
        want = golden[f"erode_out_{k}"] != 0
        assert np.array_equal(merge_ref.erode(m), want), k
        assert np.array_equal(merge_ref.erode_loop(m), want), k


def test_projection_matches_reference(golden):
    p, wt, ip, out = golden["proj_p"], golden["proj_wt"], golden["proj_ip"], golden["proj_out"]
    for k in range(len(p)):
        x, y, d = color_ref.project(p[k, 0:1], p[k, 1:2], p[k, 2:3], ip[k], wt[k])
        assert (int(x[0]), int(y[0]), int(d[0])) == tuple(int(v) for v in out[k]), k


def test_cvt_u16_x64():
    v = np.array([0.0, 0.99, 65535.0, 65535.5, 65536.0, 65537.9, -1.0, -0.5, 3e9, -3e9, np.nan, np.inf], dtype=np.float32)
    assert merge_ref.cvt_u16_x64(v).tolist() == [0, 0, 65535, 65535, 0, 1, 65535, 0, 0, 0, 0, 0]


def test_merge_keeps_vertices_and_changes_triangles(orc):
    """Four sensors facing one wall: the merge assigns vertices and drops triangles; one sensor is the reprojection alone."""
    rig = merge_cases.wall(4)
    tris, diag = merge_ref.overlay_merge(rig, orc)
    _, _, plain = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    assert diag["assigned"].sum() > 0 and len(tris) < len(plain)
    assert tris.min() >= 0 and tris.max() < diag["offsets"][-1]
    one = color_cases.ring(1, sizes=[(128, 106)], of=8)
    t1, d1 = merge_ref.overlay_merge(one, orc)
    assert d1["assigned"].sum() == 0 and np.array_equal(d1["reprojected"], d1["merged"])
