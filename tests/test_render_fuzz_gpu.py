"""Seeded rigs with random virtual cameras through lsnFusionRenderViews, mesh and points mode, against tests/render_ref.py, bit for bit."""
import numpy as np
import pytest

from livescan3d_amd import synth
from tests import render_ref, support

pytestmark = pytest.mark.gpu

SIZES = [(96, 80), (64, 48), (37, 29), (8, 8)]


def _random_view(rng, rig):
    """A sensor's pose turned by up to 25 degrees about two axes and moved by up to 0.4 m, its focal length scaled by 0.5 .. 4."""
    s = int(rng.integers(0, rig.n))
    wt = rig.wt[12 * s:12 * s + 12].astype(np.float64)
    R = wt[3:].reshape(3, 3) @ synth.rot_y(float(rng.uniform(-0.44, 0.44))) @ synth.rot_x(float(rng.uniform(-0.44, 0.44)))
    centre = wt[3:].reshape(3, 3) @ wt[:3] + rng.uniform(-0.4, 0.4, 3)
    w, h = SIZES[int(rng.integers(0, len(SIZES)))]
    intr = rig.intr[7 * s:7 * s + 7].copy()
    scale = float(rng.uniform(0.5, 4.0)) * w / float(rig.widths[s])
    intr[:4] = [(w - 1) / 2.0, (h - 1) / 2.0, intr[2] * scale, intr[3] * scale]
    return intr, render_ref.pose_at(R, centre), w, h


@pytest.mark.parametrize("seed", range(20))
def test_random_rigs_and_views(gpu, seed):
    from livescan3d_amd.fusion import DeviceFusion
    rng = np.random.default_rng(7000 + seed)
    rig = support.ring_rig(rng, 4, [4, 8], support.ragged_or_equal(96, 80, [64, 96], [48, 80]))
    intr, wt, w, h = _random_view(rng, rig)
    with DeviceFusion.from_rigs([rig]) as fus:
        fus.run_mesh()
        verts, _ = fus.tick_cloud(0)
        tris = fus.tick_triangles(0)
        for points in (False, True):
            depth, rgb = fus.render_views(intr, wt, w, h, points=points)
            wd, wc, info = render_ref.render(verts, None if points else tris, intr, wt, w, h)
            got_d, got_c = depth.cpu().numpy().view(np.uint16)[0, 0], rgb.cpu().numpy()[0, 0]
            assert np.array_equal(got_d, wd), (seed, points, int((got_d != wd).sum()))
            assert np.array_equal(got_c, wc), (seed, points)
            d = fus.plan.render_diagnostics(0, 0)
            assert d["drawn"] == info["drawn"] and d["pixels"] == info["pixels"], (seed, points, d, info)
