"""The temporal depth filter on seeded rigs (tests/temporal_cases.fuzz_case: 1..3 sensors of support.ring_rig's sizes, 2..9 ticks, a
per-pixel base with noise, jumps and about 25 % dropouts, random parameters with the extremes of alpha_q and delta among them) against the
restatement, bit for bit in maps, state and diagnostics.  tests/test_temporal_ref.py holds the generator to its branch mix on the CPU."""
import numpy as np
import pytest

from tests import temporal_cases as cases
from tests.test_temporal_gpu import Batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_seeded_rigs_equal_the_restatement(gpu, seed):
    sizes, params, maps = cases.fuzz_case(seed)
    b = Batch(sizes, maps.shape[0], shift=2 * (seed % 3 == 2))      # every third seed off 16-byte alignment
    b.plan.set_temporal(*params)
    b.check(maps, None, params, (seed, "from no history"))
    b.check(maps[::-1].copy(), None, params, (seed, "continued"), in_place=seed % 2 == 1)
    b.close()
