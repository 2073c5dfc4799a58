"""The boundary frames of tests/tri_cases.py on the CPU: a census, by the instrumented restatement of tests/tri_ref.py, that every stencil
is hit as it was built -- every (level, triangle, edge, rule, margin) of the general frame, every (triangle, edge, rule, margin, lane
column) of the VEC frame, the decisive difference exactly on thr - 1 or thr -- and that the C oracle equals the restatement, the fixture
made by the reference's own generateTrianglesGradients (tests/golden/tri_boundary_ref.npz) and, where it is built, the compiled
reference.  Conditions, not tolerances: nothing here is skipped but the live comparison with a library that cannot be built everywhere."""
import functools
import os

import numpy as np
import pytest

from tests import tri_cases, tri_ref
from tests.tri_ref import RULES

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tri_boundary_ref.npz")
BACKGROUNDS = ("holes", "dense")


@functools.lru_cache(maxsize=None)
def _frame(which, background):
    f = {"vec": tri_cases.vec_frame, "gen": tri_cases.general_frame}[which]()
    return f.with_background(background)


def _census(orc, f):
    """{placement index: trace_pixel of its P} for the placements whose P lies where triangles are made."""
    p2v = tri_cases.p2v_of(orc, f)
    out = {}
    for k, p in enumerate(f.placements):
        if 1 <= p["x"] < f.w - 2 and 2 <= p["y"] < f.h - 2:
            out[k] = tri_ref.trace_pixel(f.depth.astype(np.int64), p2v, p["x"], p["y"])
    return out


def _assert_hit_as_built(f, p, t):
    """The target of placement p is what pixel P of the frame really decides on."""
    level, i, j, rule, margin = p["label"]
    where = f.describe(p["x"], p["y"])
    assert int(f.depth[p["y"], p["x"]]) == level, where
    assert not t["skipped"], where
    tr = t["traces"][i]
    assert tr is not None, f"{where}: triangle {i} was not evaluated"
    thr, e = tr["thr"], tr["edges"][j]
    assert e[rule] == (thr - 1 if margin == "accept" else thr), (where, e, thr)
    for r in RULES:
        if r != rule:
            assert e[r] is None or e[r] >= thr, (where, r, e, thr)       # this compare alone decides the edge ...
    for k in range(3):
        if k != j:
            assert any(tr["edges"][k][r] is not None and tr["edges"][k][r] < thr for r in RULES), (where, k)   # ... and the edge the triangle
    assert t["verdicts"][i] == (margin == "accept"), where
    assert (i in t["emitted"]) == (margin == "accept"), where
    if i >= 2:
        assert not t["verdicts"][0] and not t["verdicts"][1], where


@pytest.mark.parametrize("background", BACKGROUNDS)
def test_census_general_frame_hits_every_target(orc, background):
    f = _frame("gen", background)
    census = _census(orc, f)
    hit = {}
    for k, p in enumerate(f.placements):
        if p["kind"] == "target":
            _assert_hit_as_built(f, p, census[k])
            hit[p["label"]] = census[k]
    want = {(L, i, j, r, m) for L in tri_cases.LEVELS for (i, j, r, m) in tri_cases.all_targets()}
    assert len(want) == 288 and set(hit) == want
    for (L, i, j, r, m) in want:                                          # accept and reject flip the emitted triangle
        assert (i in hit[(L, i, j, r, "accept")]["emitted"]) and (i not in hit[(L, i, j, r, "reject")]["emitted"]), (L, i, j, r)


@pytest.mark.parametrize("background", BACKGROUNDS)
def test_census_vec_frame_hits_every_target_at_every_lane_column(orc, background):
    f = _frame("vec", background)
    assert f.w == 64 and f.w * f.h <= 100_000
    census = _census(orc, f)
    hit, levels = {}, {}
    for k, p in enumerate(f.placements):
        if p["kind"] == "target":
            _assert_hit_as_built(f, p, census[k])
            hit[p["label"][1:] + (p["x"] % 8,)] = (p["label"][0], census[k])
            levels.setdefault(p["label"][1:], set()).add(p["label"][0])
    want = {t + (col,) for t in tri_cases.all_targets() for col in range(8)}
    assert len(want) == 576 and set(hit) == want
    assert all(levels[t] == set(tri_cases.LEVELS) for t in tri_cases.all_targets())
    for (i, j, r, m, col) in want:
        a, b = hit[(i, j, r, "accept", col)], hit[(i, j, r, "reject", col)]
        assert a[0] == b[0] and i in a[1]["emitted"] and i not in b[1]["emitted"], (i, j, r, col)
    # where the stencils lie: the frame's first and last columns and rows that emit, and the last lane of a row
    xs = {p["x"] for k, p in enumerate(f.placements) if k in census}
    ys = {p["y"] for k, p in enumerate(f.placements) if k in census}
    assert 1 in xs and f.w - 3 in xs and 2 in ys and f.h - 3 in ys
    assert {p["x"] % 8 for p in f.placements if p["kind"] == "target" and p["x"] >= f.w - 8} == {0, 1, 2, 3, 4, 5}
    across = [p for k, p in enumerate(f.placements) if k not in census]
    assert {(p["x"] == 0, p["x"] == f.w - 2, p["y"] == 1, p["y"] == f.h - 2) for p in across} == \
        {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}


@pytest.mark.parametrize("which,background", [(w, b) for w in ("vec", "gen") for b in BACKGROUNDS])
def test_census_exact_sum_stencils_sit_on_the_equality_of_the_division_free_compare(orc, which, background):
    """The kernel decides `metric < thr` as 18750 metric <= 17 s + 117618 (tests/test_fast_division.py).  Only a corner sum s with
    17 s + 117618 == 0 or -1 (mod 18750) can tell that compare from one whose constant is off by one or whose <= is a <: the exact-sum
    stencils have such sums, for every triangle and both margins, at every lane column of the VEC frame."""
    f = _frame(which, background)
    census = _census(orc, f)
    seen = set()
    for k, p in enumerate(f.placements):
        if p["kind"] == "exact":
            _assert_hit_as_built(f, p, census[k])
            level, i, j, rule, margin = p["label"]
            s = sum(int(f.depth[p["y"] + dy, p["x"] + dx]) for dx, dy in tri_ref.CHECK_CORNERS[i])
            m = census[k]["traces"][i]["edges"][j][rule]
            assert 18750 * m == 17 * s + 117618 + (margin == "reject"), f.describe(p["x"], p["y"])
            seen.add((i, margin, p["x"] % 8 if which == "vec" else 0))
    assert seen == {(i, m, c) for i in range(4) for m in tri_cases.MARGINS for c in (range(8) if which == "vec" else [0])}
    assert len({p["label"][0] for p in f.placements if p["kind"] == "exact"}) >= 8      # ... over many levels


@pytest.mark.parametrize("which,background", [(w, b) for w in ("vec", "gen") for b in BACKGROUNDS])
def test_census_special_stencils_emit_what_is_written_out_by_hand(orc, which, background):
    f = _frame(which, background)
    census = _census(orc, f)
    p2v = tri_cases.p2v_of(orc, f)
    # depth CUT has a vertex, every depth above it has depth and no vertex
    assert ((p2v.reshape(f.h, f.w) != -1) == ((f.depth != 0) & (f.depth <= tri_cases.CUT))).all()
    assert (f.depth > tri_cases.CUT).any()
    seen = {}
    for k, p in enumerate(f.placements):
        if p["kind"] in ("special", "lanes"):
            seen.setdefault(p["label"], []).append(census[k])
            if p["expected"] is not None:
                assert census[k]["emitted"] == p["expected"], f.describe(p["x"], p["y"])
    assert len(seen) == len(tri_cases.special_stencils()) + (which == "vec") and all(len(v) == (8 if which == "vec" else 1) for k, v in seen.items() if k != "lane_without_vertices")
    # the cases the kernel's order of masks could get wrong, once more in full:
    for t in seen["novertex_R"]:          # R cropped away: verdicts 0 and 1 are TRUE, so 2 and 3 are never evaluated, and nothing is emitted
        assert t["verdicts"] == [True, True, False, False] and t["traces"][2] is None and t["traces"][3] is None and t["emitted"] == []
    for t in seen["novertex_U"]:
        assert t["verdicts"] == [True, True, False, False] and t["emitted"] == []
    for t in seen["novertex_UR"]:
        assert t["verdicts"] == [True, True, False, False] and t["emitted"] == [0]
    for t in seen["novertex_P"] + seen["flat_65535"]:
        assert t["skipped"] and t["emitted"] == []
    for t in seen["novertex_probes"]:
        assert t["emitted"] == [0, 1]
    for t in seen["novertex_probe_decides"]:   # the probe without a vertex is what lets U - R pass
        e = t["traces"][0]["edges"][1]
        assert e["abs"] >= t["traces"][0]["thr"] and e["fwd"] == 1 and e["bwd"] is None and t["emitted"] == [0, 1]
    for t in seen["flat_1"]:
        assert t["traces"][0]["thr"] == 7 and t["emitted"] == [0, 1]
    if which == "vec":
        (t,) = seen["lane_without_vertices"]
        assert t["skipped"]
        k = [p["label"] for p in f.placements].index("lane_without_vertices")
        x, y = f.placements[k]["x"], f.placements[k]["y"]
        assert (p2v.reshape(f.h, f.w)[y, 8:16] == -1).all() and (f.depth[y, 8:16] != 0).all()
        assert tri_ref.trace_pixel(f.depth.astype(np.int64), p2v, x + 1, y)["emitted"] == [0, 1]


def test_hand_made_stencils_under_the_wide_box(orc):
    """There the windows at 65 535 have vertices: the threshold reaches 185 and a flat window emits both triangles."""
    for w in (64, 61):
        f = tri_cases.hand_frame(w)
        census = _census(orc, f)
        by = {p["label"]: census[k] for k, p in enumerate(f.placements) if p["kind"] == "special"}
        assert by["flat_65535"]["traces"][0]["thr"] == 185 and by["flat_65535"]["emitted"] == [0, 1]
        assert by["novertex_R"]["emitted"] == [0, 1]
        assert by["zero_R"]["emitted"] == [2] and by["zero_U"]["emitted"] == [3] and by["zero_P"]["skipped"]


def _all_frames():
    return [_frame(w, b) for w in ("vec", "gen") for b in BACKGROUNDS] + tri_cases.fixture_frames()[2:]


def test_c_oracle_equals_python_restatement_on_every_frame(orc):
    total = 0
    for f in _all_frames():
        p2v = tri_cases.p2v_of(orc, f)
        want = tri_ref.py_triangles(f.depth, p2v)
        got = orc.generate_triangles(f.depth, p2v)
        assert got.shape == want.shape and np.array_equal(got, want), f.name
        rig = tri_cases.rig_of([f])                                         # ... and the rig as the GPU will see it
        v, counts, tri = orc.generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds)
        assert len(v) == int((p2v != -1).sum()) and tri.shape == want.shape and np.array_equal(tri, want), f.name
        total += len(want)
    assert total > 50000


def test_write_pass_frames_hold_the_searched_counts(orc):
    for w, h in tri_cases.WRITE_SIZES:
        frames = tri_cases.write_frames(w, h)
        assert set(frames) == set(tri_cases.WRITE_COUNTS) | {"tile1"}
        for k, d in frames.items():
            f = tri_cases.frame_of(f"write{w}x{h}_{k}", d)
            p2v = tri_cases.p2v_of(orc, f)
            tri = orc.generate_triangles(d, p2v)
            # tile 0 = the first TILE pixels; the per-pixel counts of a flat frame need no depth test (tri_cases.flat_counts): the oracle is held to their sum
            counts = tri_cases.tile_counts(d)
            assert sum(counts) == len(tri), (w, h, k)
            if k == "tile1":
                assert counts[0] == 0 and counts[1] > 0
            elif k == "full":
                assert (d != 0).all() and counts[0] > 3073 and counts[1] > 0
            else:
                assert counts[0] == k and sum(counts[1:]) == 0, (w, h, k)


def test_oracle_equals_reference_fixture(orc):
    """tri_boundary_ref.npz holds the output of the reference's own generateTrianglesGradients (tests/golden/make_tri_golden.py) on
    frames that are rebuilt here: the inputs must still be the ones the fixture was made from."""
    z = np.load(GOLDEN)
    frames = tri_cases.fixture_frames()
    assert list(z["names"]) == [f.name for f in frames]
    for f in frames:
        depth, p2v, want = z[f"{f.name}_depth"], z[f"{f.name}_p2v"], z[f"{f.name}_tri"]
        assert depth.dtype == np.uint16 and np.array_equal(depth, f.depth), f.name
        assert np.array_equal(p2v, tri_cases.p2v_of(orc, f)), f.name
        got = orc.generate_triangles(depth, p2v)
        assert got.shape == want.shape and np.array_equal(got, want), f.name


def test_oracle_equals_compiled_reference_on_the_vec_frame(orc):
    """Live comparison with oracle/_ref/libref_tri.so (the reference's meshGenerator.cpp compiled as it lies), where it is built."""
    if not orc.have_ref_tri():
        pytest.skip("oracle/_ref/libref_tri.so not built (needs the reference's sources)")
    for b in BACKGROUNDS:
        f = _frame("vec", b)
        p2v = tri_cases.p2v_of(orc, f)
        got, want = orc.generate_triangles(f.depth, p2v), orc.ref_triangles(f.depth, p2v)
        assert got.shape == want.shape and np.array_equal(got, want), f.name
