"""Seeded rigs through lsnFusionFragments against tests/fragments_ref.py: the bit-exact bar of tests/test_fragments_gpu.py (check_device),
min_vertices drawn log-uniformly from [2, 200)."""
import numpy as np
import pytest

from tests import support
from tests.fragments_cases import check_device

pytestmark = pytest.mark.gpu

N_RIGS = 40
SEED0 = 12000


def draw(seed):
    """-> (rig, min_vertices) of one seed (the order of the draws is part of the cases)."""
    rng = np.random.default_rng(SEED0 + seed)
    rig = support.ring_rig(rng, 6, [4, 8], support.ragged_or_equal(64, 48, [32, 64], [24, 48]))
    min_vertices = int(np.exp(rng.uniform(np.log(2), np.log(200))))   # drawn after the rig
    return rig, min_vertices


def test_random_rigs(gpu):
    """One test for all rigs: the last assertion is about the set -- the fuzzer is not vacuous when every rig has at least 2 vertices and
    at least half of them lose some vertices but not all (with the restatement on the oracle's meshes of these seeds: 40 of 40 and 36)."""
    import torch
    from livescan3d_amd.fusion import DeviceFusion
    with_two, some = 0, 0
    for seed in range(N_RIGS):
        rig, min_vertices = draw(seed)
        with DeviceFusion.from_rigs([rig]) as fus:
            fus.run_mesh()
            _, refs = check_device(torch, fus.plan, fus.vertices, fus.offsets, fus.triangles, fus.tri_offsets, min_vertices)
        nv = len(refs[0]["remap"])
        with_two += nv >= 2
        some += 0 < refs[0]["removed_vertices"] < nv
    assert with_two == N_RIGS and 2 * some >= N_RIGS, (with_two, some)
