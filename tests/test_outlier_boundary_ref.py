"""The boundary cases of tests/outlier_boundary_cases.py on the CPU (no GPU).

Reach: every case's witness holds -- through the grid restated in the case file and the restatement's own result, the case reaches the
situation it is named for, and that situation decides a vertex.
Reference: tests/outlier_ref.py without rules equals the reference's own KNNeighbors and filter() on every block of every case, bit for
bit (tests/golden/outlier_boundary_ref.npz, made by tests/golden/make_outlier_boundary_golden.py): kDistance, the keep mask and
changedVerticesMap, in the order-statistic form and in the count form the library computes.
Sensitivity: every wrong rule of outlier_ref.RULES changes the result of the cases KILLS names for it, and no rule survives the suite.

Nothing here has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import outlier_boundary_cases as cases, outlier_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "outlier_boundary_ref.npz")
REFERENCE = os.environ.get("LIVESCAN3D_REFERENCE", "/root/reference")

# rule -> the cases that tell it apart from the filter
KILLS = {
    "lt_thr": ["pair_x_same_at", "pair_y_diff_at", "pair_z_diff_at", "pair_xy_diff_at", "pair_xz_same_at", "pair_yz_diff_at", "pair_xyz_diff_at",
               "pair_xYz_same_at", "arith_d2_fma"],
    "self_not_counted": ["pair_x_same_at", "pair_xyz_diff_below", "k1_1e-30", "k1_1e-20", "k1_5cm", "dup5_k5_sq0", "run64_k64", "cell_ppp"],
    "duplicates_once": ["dup5_k5_sq0", "dup5_k5_sqsub", "run64_k64", "run65_k65", "run129_k129", "sign_k6_sq0", "sign_k6_sqsub", "coincide_k10"],
    "thr_not_squared": ["pair_x_same_above", "pair_y_diff_above", "pair_z_diff_above", "pair_xyz_same_above", "sign_k2_1mm", "small_inf"],
    "thr_double": ["arith_thr_double", "pair_xyz_same_at"],
    "d2_double": ["arith_d2_double", "sign_k6_sq0", "edge_slack"],
    "d2_right_to_left": ["arith_d2_right_to_left"],
    "d2_fma": ["arith_d2_fma"],
    "k_plus_1": ["pair_x_diff_at", "cell_mmm", "cell_zzp", "dup5_k5_sq0", "run129_k129", "small_finite", "box_4000m", "coincide_k10"],
    "small_le_k": ["small_finite", "small_largest", "pair_x_same_at", "coincide_k10"],
    "small_removed": ["small_inf", "small_maxdist_inf"],
    "small_kept": ["small_finite", "small_spread", "small_largest", "boundaries_a", "boundaries_b", "ticks3", "coincide_k11"],
    "scope_tick": ["scope_sensors", "boundaries_a", "boundaries_b", "ticks3"],
    "scope_batch": ["scope_sensors", "scope_ticks", "boundaries_a", "boundaries_b", "ticks3"],
}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def blocks_of(g):
    """(case index, tick, sensor, points, kDistance, changedVerticesMap's values) of every block of the fixture."""
    pos = np.concatenate([[0], np.cumsum(g["block_n"])])
    for b in range(len(g["block_n"])):
        lo, hi = int(pos[b]), int(pos[b + 1])
        yield int(g["block_case"][b]), int(g["block_tick"][b]), int(g["block_sensor"][b]), g["points"][lo:hi], g["kdist"][lo:hi], g["changed"][lo:hi]


def same(a, b):
    return all(np.array_equal(x, y) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


# ---- reach -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_witness(name):
    c = cases.BY_NAME[name]
    c.witness(c)


def test_the_suite_covers_what_it_names():
    names = set(cases.NAMES)
    for d in cases.DIRECTIONS:
        assert {f"pair_{d}_{w}_{s}" for w in ("same", "diff") for s in ("at", "below", "above")} <= names
    assert len([n for n in names if n.startswith("cell_")]) == 26
    assert {"shared_lone", "shared_k_minus_1", "shared_far", "scope_sensors", "scope_ticks", "boundaries_a", "ticks3", "box_4000m",
            "coincide_k10", "small_finite", "small_largest", "small_inf", "run64_k64", "run65_k66", "run129_k129"} <= names
    tables = {cases.buckets_of(f) for c in cases.CASES for f in c.frames}
    assert {64, 128} <= tables and any(c.frames == [cases.FRAME_POW2] for c in cases.CASES) and any(c.frames == [cases.FRAME_PAST] for c in cases.CASES)
    assert all(sum(len(b) for b in t) <= 4000 for c in cases.CASES for t in c.ticks)
    assert any(len(c.ticks) == 3 for c in cases.CASES) and any(len(b) == 0 for c in cases.CASES for _, _, b in c.blocks())


def test_the_restated_hash_shares_buckets_as_often_as_claimed():
    """About a third of all lone vertices of a 64-bucket table meet one of their buckets twice: the restated hash on 2000 random cells."""
    rng = np.random.default_rng(5)
    g = cases.Grid(np.zeros((1, 3), np.float32), 0.01, cases.FRAME_64)
    hits = sum(1 for cell in rng.integers(0, 1000, (2000, 3)) if g.walk(tuple(int(v) for v in cell))[1][0] in g.walk(tuple(int(v) for v in cell))[1][1:])
    assert 500 <= hits <= 800, hits


def test_edge_slack_search_outcome():
    """The seeded search of the stated budget finds pairs that the edge's slack alone keeps in neighbouring cells; the first is a case."""
    found = cases.edge_slack_search()
    assert found is not None and found[3] == cases.EDGE_BUDGET and found[2] > 0
    assert "edge_slack" in cases.BY_NAME and cases.BY_NAME["edge_slack"].ticks[0][0].tobytes() == found[0].tobytes()


# ---- the reference's own code ----------------------------------------------------------------------------------------------------

def test_fixture_is_what_the_case_file_describes(golden):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_outlier_boundary_golden as gen
    finally:
        sys.path.pop(0)
    want = gen.layout()
    assert sorted(golden.files) == sorted(list(want) + ["kdist", "changed"])
    for key, a in want.items():
        assert golden[key].dtype == a.dtype and golden[key].shape == a.shape and golden[key].tobytes() == a.tobytes(), key
    assert len(golden["kdist"]) == len(golden["changed"]) == len(golden["points"])
    assert len(set(golden["block_case"].tolist())) == len(cases.CASES)          # every case ran on the reference
    assert os.path.getsize(GOLDEN) < 500 * 1024


def test_restatement_equals_the_reference_on_every_block(golden):
    n_blocks = 0
    for ci, t, s, pts, kd, changed in blocks_of(golden):
        c = cases.CASES[ci]
        what = (c.name, t, s)
        assert pts.tobytes() == c.ticks[t][s].tobytes(), what
        assert ref.k_distance(pts, c.k).tobytes() == kd.tobytes(), what
        keep = changed >= 0
        assert np.array_equal(changed[keep], np.arange(keep.sum())), what
        assert np.array_equal(ref.keep_mask(pts, c.k, c.max_dist), keep), what
        assert np.array_equal(ref.keep_mask(pts, c.k, c.max_dist, brute_limit=0), keep), what          # the count form
        assert np.array_equal(c.keep()[t][s], keep) and np.array_equal(c.keep(brute_limit=0)[t][s], keep), what
        n_blocks += 1
    assert n_blocks == sum(len(c.blocks()) for c in cases.CASES) >= 150


def test_generator_reproduces_the_fixture(tmp_path):
    """Reruns the reference on every block where a checkout is present (the only test here that reads it): identical arrays."""
    if not os.path.exists(os.path.join(REFERENCE, "src", "LiveScanClient", "filter.cpp")):
        pytest.skip("no LiveScan3D checkout at $LIVESCAN3D_REFERENCE; the committed fixture stands for it")
    gen = os.path.join(HERE, "golden", "make_outlier_boundary_golden.py")
    subprocess.check_call([sys.executable, gen, REFERENCE, str(tmp_path)], stdout=subprocess.DEVNULL, timeout=600)
    fresh, z = np.load(tmp_path / "outlier_boundary_ref.npz"), np.load(GOLDEN)
    assert sorted(fresh.files) == sorted(z.files)
    for k in z.files:
        assert fresh[k].dtype == z[k].dtype and fresh[k].tobytes() == z[k].tobytes(), k


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rule", sorted(ref.RULES))
def test_rule_is_killed_by_the_cases_named_for_it(rule):
    assert KILLS[rule]
    for name in KILLS[rule]:
        c = cases.BY_NAME[name]
        assert not same(c.keep(), c.keep(rules=[rule])), (rule, name)


def test_no_rule_survives_the_suite():
    assert set(KILLS) == set(ref.RULES)
    for rule in ref.RULES:
        killers = [c.name for c in cases.CASES if not same(c.keep(), c.keep(rules=[rule]))]
        print(f"{rule:18s} {ref.RULES[rule]:62s} <- {len(killers)} cases")
        assert killers and set(KILLS[rule]) <= set(killers), rule


def test_without_rules_nothing_changes():
    for c in cases.CASES:
        for t, s, b in c.blocks():
            assert np.array_equal(ref.keep_mask(b, c.k, c.max_dist, rules=()), ref.keep_mask(b, c.k, c.max_dist))
            assert ref.k_distance(b, c.k, rules=None).tobytes() == ref.wrong_k_distance(b, c.k).tobytes()      # the rules' own path, no rule on
    with pytest.raises(AssertionError):
        ref.keep_mask(np.zeros((3, 3), np.float32), 2, 0.1, rules=["no_such_rule"])
