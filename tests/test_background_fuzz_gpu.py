"""Background subtraction on seeded rigs (tests/background_cases.fuzz_case: 1..8 sensors, 1..5 ticks, a room with unseen pixels learned from
two ticks, subjects and specks in front of it, dropouts, random settings with the extremes of margin and rel_q among them) against the
restatement, bit for bit in model, maps and diagnostics.  tests/test_background_ref.py holds the generator to its mix on the CPU: kept,
background and unknown pixels, removed and surviving components, a component across two tiles, on every seed."""
import numpy as np
import pytest

from tests import background_cases as cases, background_ref as ref
from tests.test_background_gpu import Batch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", cases.FUZZ_SEEDS)
def test_seeded_rigs_equal_the_restatement(gpu, seed):
    sizes, params, room, maps = cases.fuzz_case(seed)
    shift = 2 * (seed % 3 == 2)                                     # every third seed off 16-byte alignment
    lb = Batch(sizes, room.shape[0], shift)
    model = lb.learn(room)
    assert np.array_equal(model, ref.learn(np.zeros(lb.px, np.uint16), room)), seed
    lb.close()
    b = Batch(sizes, maps.shape[0], shift)
    b.plan.set_background(*params)
    b.check(maps, model, params, seed, in_place=seed % 2 == 1)
    b.close()
