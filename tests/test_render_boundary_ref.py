"""The render stage's definition (tests/render_ref.py, numpy) on the hand-made cases of tests/render_boundary_cases.py, without a GPU:
held byte for byte to the plain-Python loops (tests/render_ref_py.py), every case to its witness -- what it is named for is reached,
read from the definition's own terms -- and to the mutants it is listed to kill.  Suite conditions: every case that is not named a
no-op draws at least one pixel, the no-ops none; every mutant of render_ref_py.RULES is killed by some case."""
import numpy as np
import pytest

from tests import render_boundary_cases as cases, render_ref as ref, render_ref_py as ref_py

LOOPED = tuple(n for n in cases.NAMES if n not in cases.NUMPY_ONLY)
_results = {}


def _tris(c, t):
    return None if c.points else (np.zeros((0, 3), np.int32) if t is None else t)


def _result(name):
    """Per tick and view of a case: (depth, rgb, info, terms) of the definition.  Computed once, never changed."""
    if name not in _results:
        c, out = cases.case(name), []
        for v, t in c.ticks:
            row = []
            for q in range(len(c.intr)):
                terms = []
                depth, rgb, info = ref.render(v, _tris(c, t), c.intr[q], c.wt[q], c.w, c.h, terms=terms)
                for a in (depth, rgb, info["boxes"]):
                    a.setflags(write=False)
                row.append((depth, rgb, info, terms[0]))
            out.append(row)
        _results[name] = out
    return _results[name]


def _loops(name, rules=(), terms=None):
    c = cases.case(name)
    return [[ref_py.render(v, _tris(c, t), c.intr[q], c.wt[q], c.w, c.h, rules=rules, terms=terms) for q in range(len(c.intr))] for v, t in c.ticks]


def _same(a, b):
    return all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2]["drawn"] == y[2]["drawn"]
               and x[2]["pixels"] == y[2]["pixels"] and np.array_equal(x[2]["boxes"], y[2]["boxes"]) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.mark.parametrize("name", LOOPED)
def test_numpy_equals_the_python_loops(name):
    terms = []
    got = _loops(name, terms=terms)
    want = _result(name)
    assert _same(want, got), name
    # and their intermediate values: the projection of every vertex, the candidates of every pixel with their vals
    for (_, _, _, a), b in zip((r for row in want for r in row), terms):
        assert [a[k].tolist() for k in "xyd"] == [b[k] for k in "xyd"] and a["ok"].tolist() == b["ok"]
        if not cases.case(name).points:
            mine = sorted(zip(a["ck"].tolist(), a["cx"].tolist(), a["cy"].tolist(), a["cval"].tolist(), a["cw1"].tolist(), a["cw2"].tolist(), a["cw3"].tolist()))
            assert mine == sorted((t, x, y, v, float(w1), float(w2), float(w3)) for t, x, y, v, w1, w2, w3 in b["cand"])


def test_the_two_without_loops_say_why():
    assert set(cases.NUMPY_ONLY) == {"raster_two_pass", "budget_1024"} and set(cases.NUMPY_ONLY) < set(cases.NAMES)


@pytest.mark.parametrize("name", cases.NAMES)
def test_witness(name):
    c, res = cases.case(name), _result(name)
    c.witness(c, res if c.every_view else [row[c.view] for row in res])


@pytest.mark.parametrize("name", cases.NAMES)
def test_a_case_draws_unless_it_is_named_a_noop(name):
    c = cases.case(name)
    drawn = sum(r[2]["pixels"] for row in _result(name) for r in (row if c.every_view else row[c.view:c.view + 1]))
    assert (drawn == 0) == c.noop, (name, drawn)
    if c.noop:
        assert all(not r[0].any() and not r[1].any() for row in _result(name) for r in row)


@pytest.mark.parametrize("name", LOOPED)
def test_the_listed_mutants_are_killed(name):
    """(Killed: the image or a count differs; tests/render_boundary_cases.py says where it is a count alone.  A case that lists none
    has nothing to show here.  The cases are built inside the tests, never when the file is collected.)"""
    right = _loops(name)
    for rule in cases.case(name).kills:
        assert not _same(right, _loops(name, rules=(rule,))), (name, rule, ref_py.RULES[rule])


def test_every_mutant_is_killed_by_some_case():
    killed = {r for n in LOOPED for r in cases.case(n).kills}
    assert killed == set(ref_py.RULES), set(ref_py.RULES) ^ killed


def test_an_unknown_rule_is_refused():
    c = cases.case("one_pixel")
    with pytest.raises(AssertionError):
        ref_py.render(*c.ticks[0], c.intr[0], c.wt[0], c.w, c.h, rules=("no_such_rule",))
