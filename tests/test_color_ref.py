"""The CPU reference of the colour transfer (tests/color_ref.py), no GPU needed:
  * its Reinhard part (transform + apply) bit for bit against the reference's own colorcorrection.cpp (tests/golden/color_transfer_ref.npz,
    made by tests/golden/make_color_golden.py): random, empty, single-sample, constant-colour sets and every value of every channel;
  * the whole stage against the independent plain-Python restatement (tests/color_ref_py.py) on small random rigs;
  * the confidence map's shift_x row bug, and the x64 conversion rule."""
import os

import numpy as np
import pytest

from livescan3d_amd import synth
from tests import color_cases, color_ref, color_ref_py

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_transfer_ref.npz")


def test_reinhard_part_matches_reference_colorcorrection():
    z = np.load(GOLDEN)
    n = int(z["n_cases"])
    assert n >= 13
    every = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    for k in range(n):
        xf = color_ref.transform(z[f"src_{k}"], z[f"dst_{k}"])
        assert xf.tobytes() == z[f"xform_{k}"].tobytes(), (k, xf, z[f"xform_{k}"])
        assert np.array_equal(color_ref.apply(every, xf), z[f"applied_{k}"]), k


def test_constant_colour_goes_to_zero_as_on_x64():
    """A constant-colour sample set makes scale ~ 1e15: every other value is out of int range and becomes 0 (x64), not 255 (saturation)."""
    z = np.load(GOLDEN)
    k = next(k for k in range(int(z["n_cases"])) if len(z[f"dst_{k}"]) and (z[f"dst_{k}"] == z[f"dst_{k}"][0]).all()
             and not (z[f"src_{k}"] == z[f"src_{k}"][0]).all())
    assert z[f"xform_{k}"][6:].min() > 1e12
    out = z[f"applied_{k}"]
    c = int(z[f"dst_{k}"][0, 0])
    assert (out[np.arange(256) != c] == 0).all()
    assert color_ref.cvt_i32_x64(np.array([np.nan, 1e300, -1e300, 2147483647.9, -2147483648.9, -0.9])).tolist() == \
        [-2 ** 31, -2 ** 31, -2 ** 31, 2147483647, -2147483648, 0]


def _correct_8_neighbour_seeds(d):
    h, w = d.shape
    d = d.astype(np.int64)
    seeds = np.zeros((h, w), bool)
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            if d[y, x] == 0:
                continue
            nb = d[y - 1:y + 2, x - 1:x + 2]
            seeds[y, x] = bool(((np.abs(nb - d[y, x]) > 20) | (nb == 0)).any())
    return seeds


def test_confidence_keeps_the_shift_x_row_bug():
    a, b = color_cases.shift_x_frames()
    ca, cb = color_ref.confidence_map(a), color_ref.confidence_map(b)
    assert np.array_equal(cb, np.array(color_ref_py.confidence(b), np.uint8).reshape(b.shape))
    assert np.array_equal(ca, np.array(color_ref_py.confidence(a), np.uint8).reshape(a.shape))
    # the step along x - y = 10 seeds nothing with the reference's probes, but would with a true 8-neighbour test
    step = (np.abs(np.subtract.outer(np.arange(48), np.arange(64)) + 10) <= 1)   # pixels next to the diagonal
    assert _correct_8_neighbour_seeds(b)[step].any()
    assert not (cb[step] == 1).any()


@pytest.mark.parametrize("seed", range(6))
def test_confidence_numpy_matches_loops(seed):
    rng = np.random.default_rng(seed)
    h, w = rng.integers(1, 40, 2)
    d = rng.integers(900, 960, (h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.05] = 0
    d[:, : w // 3] += 200
    assert np.array_equal(color_ref.confidence_map(d), np.array(color_ref_py.confidence(d), np.uint8).reshape(h, w))


def _same(a, b):
    va, da = a
    vb, db = b
    assert va.tobytes() == vb.tobytes()
    assert np.array_equal(da["confidence"], db["confidence"])
    assert np.array_equal(da["coverage"], db["coverage"])
    assert da["pairs"] == db["pairs"]
    assert da["transforms"].tobytes() == db["transforms"].tobytes()


@pytest.mark.parametrize("seed", range(3))
def test_reference_matches_plain_python_on_small_rigs(orc, seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(2, 4))
    sizes = [(int(rng.integers(200, 240)), int(rng.integers(160, 190))) for _ in range(n)]
    bounds = np.array([-1.5, -1.0, -1.5, 1.5, 1.5, float(rng.uniform(0.3, 1.5))], np.float32)
    rig = color_cases.ring(n, sizes=sizes, bounds=bounds, seed=seed + 11, of=12)
    want = color_ref.color_transfer(rig, orc)
    _same(want, color_ref_py.color_transfer(rig, orc))
    if seed == 0:
        assert want[1]["pairs"], "the rig should have overlapping views"


def test_reference_on_edge_rigs_matches_plain_python(orc):
    for rig in (color_cases.disjoint_pairs(96, 80), color_cases.no_overlap(96, 80),
                color_cases.ring(3, sizes=[(1, 1), (37, 29), (61, 47)])):
        _same(color_ref.color_transfer(rig, orc), color_ref_py.color_transfer(rig, orc))
