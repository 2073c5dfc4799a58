"""Seeded rigs through lsnFusionSimplify, mesh and points mode, against tests/simplify_ref.py: the bit-exact bar of
tests/test_simplify_gpu.py (check_device), the cell drawn log-uniformly from [0.02, 0.3]."""
import numpy as np
import pytest

from tests import support
from tests.simplify_cases import check_device

pytestmark = pytest.mark.gpu

N_RIGS = 40
SEED0 = 9000


def draw(seed):
    """-> (rig, cell, points) of one seed (the order of the draws is part of the cases)."""
    rng = np.random.default_rng(SEED0 + seed)
    rig = support.ring_rig(rng, 6, [4, 8], support.ragged_or_equal(64, 48, [32, 64], [24, 48]))
    cell = float(np.exp(rng.uniform(np.log(0.02), np.log(0.3))))
    return rig, cell, seed % 2 == 1


def test_random_rigs(gpu):
    """One test for all rigs: the last assertion is about the set -- the fuzzer is not vacuous when at least half of the rigs with at
    least 2 vertices lose vertices (confirmed with the restatement on the CPU for these seeds: 37 of the 39 such rigs do)."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    with_two, fewer = 0, 0
    for seed in range(N_RIGS):
        rig, cell, points = draw(seed)
        with DeviceFusion.from_rigs([rig]) as fus:
            fus.run_mesh()
            _, refs = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, cell, points)
        nv = len(refs[0]["remap"])
        with_two += nv >= 2
        fewer += nv >= 2 and refs[0]["cells"] < nv
    assert with_two >= N_RIGS // 2 and 2 * fewer >= with_two, (with_two, fewer)
