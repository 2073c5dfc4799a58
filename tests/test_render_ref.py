"""The CPU restatement of the render stage (tests/render_ref.py): its pixel walk against merge_ref's, its z-buffer against the reference's own
drawTriangle depth maps (tests/golden/overlay_merge_ref.npz), and the properties the stage is defined by.  No GPU."""
import os

import numpy as np
import pytest

from tests import color_cases, color_ref, merge_ref, render_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlay_merge_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def ring_mesh(orc):
    rig = color_cases.ring(3, sizes=[(96, 80)] * 3)
    v, _, t = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
    return rig, v, t


def test_pixel_walk_equals_merge_ref(golden):
    for k in range(int(golden["n_draw"])):
        s = merge_ref.triangle_setup(*golden[f"draw_tris_{k}"].astype(np.int64).T)
        a, b = render_ref.walk(s), merge_ref.triangle_pixels(s)
        for got, want in zip(a[:4], b):
            assert np.array_equal(got, want), k
        assert all(w.dtype == np.float32 for w in a[4:])


def test_z_buffer_reproduces_the_reference_depth_maps(golden):
    """What ties the defined semantics to the reference's drawTriangle: vertices that project exactly onto the golden triangles'
    integer corners, rendered, give the depth maps the reference's own loop left -- in all eight cases."""
    W, H = (int(v) for v in golden["size"])
    intr = render_ref.intrinsics(W, H)
    for k in range(int(golden["n_draw"])):
        v, t = render_ref.soup(golden[f"draw_tris_{k}"], intr)
        depth, rgb, info = render_ref.render(v, t, intr, render_ref.IDENTITY, W, H)
        assert np.array_equal(depth, golden[f"draw_depth_{k}"]), k
        assert info["pixels"] == int((golden[f"draw_depth_{k}"] != 0).sum())
        assert not rgb[depth == 0].any()


def test_order_independence(golden):
    W, H = (int(v) for v in golden["size"])
    intr = render_ref.intrinsics(W, H)
    rng = np.random.default_rng(3)
    for k in (0, 5, 7):
        t9 = golden[f"draw_tris_{k}"]
        v, t = render_ref.soup(t9, intr, rng.integers(0, 256, (3 * len(t9), 3)))
        want = render_ref.render(v, t, intr, render_ref.IDENTITY, W, H)
        order = rng.permutation(len(t))
        got = render_ref.render(v, t[order], intr, render_ref.IDENTITY, W, H, labels=order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), k


def test_ties_go_to_the_lower_index():
    intr = render_ref.intrinsics(32, 24)
    one = [2, 2, 900, 5, 20, 900, 28, 3, 900]
    v, t = render_ref.soup([one, one], intr, [[255, 0, 0]] * 3 + [[0, 0, 255]] * 3)
    d, rgb, _ = render_ref.render(v, t, intr, render_ref.IDENTITY, 32, 24)
    assert (d != 0).sum() > 100 and set(map(tuple, rgb[d != 0])) == {(255, 0, 0)}
    d2, rgb2, _ = render_ref.render(v, t[::-1], intr, render_ref.IDENTITY, 32, 24)   # the blue one first
    assert np.array_equal(d, d2) and set(map(tuple, rgb2[d2 != 0])) == {(0, 0, 255)}


def test_colour_stays_in_range_at_0_and_255():
    intr = render_ref.intrinsics(64, 48)
    rng = np.random.default_rng(9)
    xy = np.stack([rng.integers(0, 64, (200, 3)), rng.integers(0, 48, (200, 3))], axis=2)
    t9 = np.concatenate([xy, rng.integers(400, 60000, (200, 3, 1))], axis=2).reshape(200, 9)
    for c in (0, 255):
        v, t = render_ref.soup(t9, intr, np.full((600, 3), c))
        d, rgb, _ = render_ref.render(v, t, intr, render_ref.IDENTITY, 64, 48)
        assert (d != 0).sum() > 500 and (rgb[d != 0] == c).all()
    # mixed colours: every channel lies between the smallest and the largest vertex value
    v, t = render_ref.soup(t9, intr, rng.choice([0, 255], (600, 3)))
    d, rgb, _ = render_ref.render(v, t, intr, render_ref.IDENTITY, 64, 48)
    assert rgb.min() == 0 and rgb.max() == 255 and len(np.unique(rgb)) > 20


def test_views_of_a_ring(ring_mesh):
    rig, v, t = ring_mesh
    views = render_ref.ring_views(rig)
    intr = np.tile(rig.intr[:7], 4)
    depth, rgb, info = render_ref.render_views(v, t, intr, views, 96, 80)
    own = np.ascontiguousarray(rig.depth_maps).view("<u2")[:96 * 80].reshape(80, 96)
    both = (depth[0] != 0) & (own != 0)
    assert both.sum() > 1500 and np.median(np.abs(depth[0][both].astype(int) - own[both].astype(int))) <= 2   # the sensor sees itself
    assert info[1]["pixels"] > 1500
    assert not depth[3].any() and not rgb[3].any() and info[3]["drawn"] == 0                                   # looking away
    # inside the scene: something is drawn, and what lies behind the camera is not
    x, y, d, ok = render_ref.project_view(v, intr[:7], views[2], 96, 80)
    R, tt = color_ref._inverse(views[2])
    behind = (np.stack([v["X"], v["Y"], v["Z"]], axis=1) @ R.T + tt)[:, 2] <= 0
    assert behind.sum() > 100 and not ok[behind].any() and info[2]["pixels"] > 500
    pts = render_ref.render(v, None, intr[:7], views[2], 96, 80)
    assert pts[2]["drawn"] == int(ok.sum()) and 0 < pts[2]["pixels"] <= pts[2]["drawn"]


def test_tiny_and_wide_views(ring_mesh):
    rig, v, t = ring_mesh
    views = render_ref.ring_views(rig)
    for w, h in ((1, 1), (1024, 3)):
        intr = render_ref.TINY_INTR[(w, h)]
        for tris in (t, None):
            d, rgb, info = render_ref.render(v, tris, intr, views[1], w, h)
            assert d.shape == (h, w) and rgb.shape == (h, w, 3)
            assert info["pixels"] > 0 or (tris is not None and w == 1)   # three vertices in one pixel are no triangle (den == 0)
    with pytest.raises(AssertionError):
        render_ref.render(v, t, render_ref.intrinsics(1025, 3), views[0], 1025, 3)


def test_out_of_range_indices_and_empty_inputs(ring_mesh):
    rig, v, t = ring_mesh
    intr, view = rig.intr[:7], render_ref.ring_views(rig)[1]
    want = render_ref.render(v, t, intr, view, 96, 80)
    bad = np.concatenate([t, [[0, 1, len(v)], [-1, 2, 3], [2 ** 30, 0, 1]]]).astype(np.int32)
    got = render_ref.render(v, bad, intr, view, 96, 80)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2]["drawn"] == want[2]["drawn"]
    for tris in (np.zeros((0, 3), np.int32), None):
        d, rgb, info = render_ref.render(v[:0], tris, intr, view, 96, 80)
        assert not d.any() and not rgb.any() and info["drawn"] == 0
