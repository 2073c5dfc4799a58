"""The outlier filter's restatement (tests/outlier_ref.py) held to the reference's own KNNeighbors and filter() over nanoflann
(tests/golden/outlier_filter_ref.npz, made by tests/golden/make_outlier_golden.py): kDistance of every point, the keep mask,
changedVerticesMap and the filtered vertices and colours, bit for bit -- oracle sensor blocks, Gaussian clusters with far outliers,
duplicates, a lattice of ties, k in {1, 2, 10, n, n + 1}, maxDist at a recorded kDistance and one float step either side, thr = inf and
the largest finite thr, k <= 0, maxDist <= 0 and NaN.  Also: the count form the library computes equals the order statistic."""
import os

import numpy as np
import pytest

from tests import outlier_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outlier_filter_ref.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(g):
    names = [str(x) for x in g["cloud_names"]]
    for c in range(len(g["case_k"])):
        name = names[int(g["case_cloud"][c])]
        yield c, name, g[f"cloud_{name}"], g[f"colors_{name}"], int(g["case_k"][c]), float(g["case_max_dist"][c])


def test_fixture_covers_the_cases(golden):
    names = [str(x) for x in golden["cloud_names"]]
    assert {"scene_block", "ring_block", "wall_block", "gauss_outliers", "duplicates", "lattice"} <= set(names)
    seen = set()
    for c, name, pts, _, k, d in _cases(golden):
        n = len(pts)
        thr = ref.threshold(d)
        seen.add(("k", k if k in (1, 2, 10) else ("n" if k == n else ("n+1" if k == n + 1 else ("le0" if k <= 0 else k)))))
        if np.isinf(thr):
            seen.add("thr_inf")
        if np.isfinite(thr) and thr > np.float32(3.4e38):   # the largest finite float square (FLT_MAX itself is no float's square)
            seen.add("thr_largest_finite")
        if np.isnan(d):
            seen.add("nan")
        if d <= 0:
            seen.add("d_le0")
        if k >= 1 and f"filtered_vertices_{c}" in golden.files and np.any(golden[f"kdist_{name}_{k}"] == thr):
            seen.add("thr_at_kdistance")
        r = golden[f"changed_{c}"]
        if len(r) and 0 < (r >= 0).sum() < n:
            seen.add("some_removed")
    for want in [("k", 1), ("k", 2), ("k", 10), ("k", "n"), ("k", "n+1"), ("k", "le0"), "thr_inf", "thr_largest_finite", "nan", "d_le0",
                 "thr_at_kdistance", "some_removed"]:
        assert want in seen, want
    assert os.path.getsize(GOLDEN) < 500 * 1024


def test_kdistance_matches_reference(golden):
    names = [str(x) for x in golden["cloud_names"]]
    n_checked = 0
    for name in names:
        pts = golden[f"cloud_{name}"]
        for key in [f for f in golden.files if f.startswith(f"kdist_{name}_")]:
            k = int(key.rsplit("_", 1)[1])
            assert ref.k_distance(pts, k).tobytes() == golden[key].tobytes(), key
            n_checked += 1
    assert n_checked >= 30


def test_filter_matches_reference(golden):
    """keep mask, changedVerticesMap and the filtered arrays of every case."""
    for c, name, pts, colors, k, d in _cases(golden):
        n = len(pts)
        changed = golden[f"changed_{c}"]
        v, col, m = ref.filter(pts, colors, k, d)
        assert m[-1] == -1
        if len(changed) == 0:   # the early return: {-1: -1} alone, nothing removed
            assert m == {-1: -1} and len(v) == n, (c, name, k, d)
            assert ref.keep_mask(pts, k, d).all()
            continue
        got = np.array([m[i] for i in range(n)], dtype=np.int32)
        assert np.array_equal(got, changed), (c, name, k, d)
        keep = changed >= 0
        assert np.array_equal(ref.keep_mask(pts, k, d), keep), (c, name, k, d)
        assert np.array_equal(ref.keep_mask(pts, k, d, brute_limit=0), keep), (c, name, k, d)   # the count form too
        if f"filtered_vertices_{c}" in golden.files:
            assert v.tobytes() == golden[f"filtered_vertices_{c}"].tobytes(), (c, name, k, d)
            assert np.asarray(col, np.uint8).tobytes() == golden[f"filtered_colors_{c}"].tobytes(), (c, name, k, d)


def test_threshold_is_the_float_product():
    for d in (0.1, 0.01, 0.0123, 3.7, 1e-20, 1e18):
        assert ref.threshold(d) == np.float32(np.float64(np.float32(d)) ** 2)
    assert np.isinf(ref.threshold(1e30))


def test_count_form_on_random_clouds_with_ties():
    """Beyond the fixture: the count form against the order statistic on more random clouds and thresholds."""
    rng = np.random.default_rng(9)
    for trial in range(6):
        pts = rng.normal(0, 0.05, (int(rng.integers(20, 700)), 3)).astype(np.float32)
        pts = np.concatenate([pts, pts[: len(pts) // 5]])   # duplicates
        for k in (1, 3, 10, len(pts)):
            kd = ref.k_distance(pts, k)
            for v in (kd[0], kd[len(kd) // 2], kd.max()):
                if not 0 < v < ref.FLT_MAX:
                    continue
                thr = np.float32(v)
                want = ~(kd > thr)
                assert np.array_equal(ref.neighbour_counts(pts, thr) >= k, want), (trial, k)
