"""Seeded fuzz of lsnFusionSmooth against tests/smooth_ref.py, the bit-exact bar of tests/test_smooth_gpu.py (check_device): rigs of the
ring fuzzer through run_mesh, plain and after lsnFusionSimplify with a random cell, with random parameters; and random index soups -- few
vertices, many triangles, indices out of range and repeated, coordinates that are not finite or beyond 4096."""
import numpy as np
import pytest

from tests import color_cases, support
from tests.simplify_ref import cloud
from tests.smooth_cases import Clouds, check_device

pytestmark = pytest.mark.gpu

N_RIGS = 12
SEED0 = 21000


def draw_params(rng):
    """(iterations, lambda, mu, pin_boundary): the ends of the ranges now and then, mu == 0 in a quarter of the draws."""
    it = int(rng.choice([1, 2, 3, 5, 10]))
    lam = float(rng.choice([1.0, 2.0 ** -10, float(rng.uniform(0.05, 1.0))], p=[0.1, 0.1, 0.8]))
    mu = float(rng.choice([0.0, -1.0, float(-rng.uniform(0.05, 1.0))], p=[0.25, 0.1, 0.65]))
    return it, lam, mu, bool(rng.random() < 0.6)


def draw(seed):
    """-> (rig, cell, parameters) of one seed (the order of the draws is part of the cases)."""
    rng = np.random.default_rng(SEED0 + seed)
    rig = support.ring_rig(rng, 5, [4, 8], support.ragged_or_equal(64, 48, [32, 64], [24, 48]))
    cell = float(np.exp(rng.uniform(np.log(0.02), np.log(0.3))))
    params = draw_params(rng)
    if seed % 4 == 1:      # an inverted crop box: no vertex survives
        rig.bounds = rig.bounds[[3, 4, 5, 0, 1, 2]].copy()
    if seed % 6 == 2:      # a NaN in the first sensor's translation: its vertices stay, with a NaN coordinate
        rig.wt = rig.wt.copy()
        rig.wt[0] = np.nan
    if seed % 6 == 5:      # a zero focal length: infinite and NaN coordinates
        rig.intr = rig.intr.copy()
        rig.intr[2] = 0.0
    return rig, cell, params


def test_random_rigs(gpu):
    """One test for all rigs: the last assertions are about the set -- the fuzzer is not vacuous when most rigs have triangles, some are
    empty, some carry triangles that are skipped for a vertex that is not finite, and both pinned and free runs occur."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    with_triangles = empty = with_skipped = simplified = pinned = free = 0
    rigs = [draw(seed) for seed in range(N_RIGS)] + [(color_cases.ring(3, sizes=[(37, 17), (1, 1), (17, 37)]), 0.05, (2, 0.5, -0.53, True))]
    for rig, cell, params in rigs:
        with DeviceFusion.from_rigs([rig]) as fus:
            fus.run_mesh()
            _, refs = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, *params)
            v, off, t, toff, _ = fus.simplify(cell)
            _, lod = check_device(torch, fus.plan, v, off, t, toff, *params)
        with_triangles += refs[0]["used"] > 0
        empty += len(refs[0]["vertices"]) == 0
        with_skipped += refs[0]["skipped"] > 0
        simplified += 0 < len(lod[0]["vertices"]) < len(refs[0]["vertices"])
        pinned += refs[0]["pinned"] > 0
        free += refs[0]["used"] > 0 and not params[3]
    print("rigs with triangles / empty / with skipped triangles / that lost vertices / pinned / free:", with_triangles, empty, with_skipped, simplified,
          pinned, free)
    assert with_triangles >= N_RIGS // 2 and empty >= 1 and with_skipped >= 1 and simplified >= N_RIGS // 3 and pinned >= 2 and free >= 1, \
        (with_triangles, empty, with_skipped, simplified, pinned, free)


def soup(rng, cap):
    """One tick of a plan with `cap` vertices: 3 .. cap vertices, up to 2 cap triangles of random indices (a tenth of them drawn from
    [-2, nv + 2), so out of range now and then; repeats come by themselves), coordinates of mixed magnitude with a few that are NaN,
    infinite or at and beyond +-4096."""
    nv = int(rng.integers(3, cap + 1))
    nt = int(rng.integers(0, 2 * cap + 1))
    tri = rng.integers(0, nv, (nt, 3))
    wild = rng.random(nt) < 0.1
    tri[wild] = rng.integers(-2, nv + 2, (int(wild.sum()), 3))
    xyz = rng.uniform(-1, 1, (nv, 3)) * 10.0 ** rng.integers(-12, 4, (nv, 1))
    bad = rng.random((nv, 3)) < 0.02
    xyz[bad] = rng.choice([np.nan, np.inf, -np.inf, 4096.0, -4096.0, 5000.0, 4095.9], int(bad.sum()))
    return cloud(xyz), np.array([0, nv], np.int32), tri.astype(np.int32), np.array([0, nt], np.int32)


def test_random_index_soups(gpu):
    """Eight ticks of soup per plan (8 x 8: 64 vertices / 128 triangles; 20 x 16: 320 / 640), each plan under three random settings."""
    import torch
    rng = np.random.default_rng(SEED0 + 500)
    skipped = used = pinned = 0
    for size, cap in (((8, 8), 64), ((20, 16), 320)):
        c = Clouds(torch, [soup(rng, cap) for _ in range(8)], sizes=(size,))
        for _ in range(3):
            _, refs = check_device(torch, c.plan, c.v, c.off, c.t, c.toff, *draw_params(rng))
            skipped += sum(r["skipped"] for r in refs)
            used += sum(r["used"] for r in refs)
            pinned += sum(r["pinned"] for r in refs)
        c.close()
    assert skipped > 100 and used > 1000 and pinned > 50, (skipped, used, pinned)
