"""lsnFusionRenderViews on the hand-made cases of tests/render_boundary_cases.py, against the definition (tests/render_ref.py).  Bit for
bit: every depth and colour byte of every tick and view, `drawn` and `pixels` of every slot's diagnostics, and `large` = the number of
drawn triangles whose box exceeds SMALL_BOX, the boxes taken from the restatement.  Outputs lie between guard bands and are prefilled
(tests.support.Clouds).  tests/test_render_boundary_ref.py holds the cases to what they claim to reach and to the mutants they kill,
without a GPU.  The small cases are the ticks of one plan per view set; every tick is drawn in mesh mode and in points mode."""
import numpy as np
import pytest

from tests import render_boundary_cases as cases, render_ref as ref
from tests.support import Clouds

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(name, points, intr=None, wt=None):
    """The definition's (depth, rgb, info) of a case, tick by tick and view by view, in one mode.  Computed once, never changed."""
    key = (name, points, None if intr is None else (intr.tobytes(), wt.tobytes()))
    if key not in _refs:
        c, out = cases.case(name), []
        intr, wt = (c.intr, c.wt) if intr is None else (intr, wt)
        for v, t in c.ticks:
            for q in range(len(intr)):
                depth, rgb, info = ref.render(v, None if points else (np.zeros((0, 3), np.int32) if t is None else t), intr[q], wt[q], c.w, c.h)
                for a in (depth, rgb, info["boxes"]):
                    a.setflags(write=False)
                out.append((depth, rgb, info))
        _refs[key] = out
    return _refs[key]


def _check(clouds, names, points, intr=None, wt=None):
    """One render of the plan whose ticks are the ticks of `names`, in order, against their references."""
    c0 = cases.case(names[0])
    intr, wt = (c0.intr, c0.wt) if intr is None else (intr, wt)
    refs = [r for n in names for r in _ref(n, points, intr, wt)]
    slots = [(n, k, q) for n in names for k in range(len(cases.case(n).ticks)) for q in range(len(intr))]
    try:
        _, _, diags = clouds.check(intr, wt, c0.w, c0.h, points=points, refs=refs)
    except AssertionError as ex:      # Clouds names the plan's tick and the view: say which case that is
        k, q = ex.args[0][:2] if ex.args and isinstance(ex.args[0], tuple) else (None, None)
        tick_of = [n for n in names for _ in cases.case(n).ticks]
        raise AssertionError(f"case {tick_of[k] if k is not None else '?'} (plan tick {k}, view {q}, {'points' if points else 'mesh'}): {ex}") from ex
    assert len(diags) == len(refs) == len(slots)
    for slot, d, (_, _, info) in zip(slots, diags, refs):
        assert d["large"] == int((info["boxes"] > cases.SMALL_BOX).sum()), (slot, d, info["boxes"].tolist()[:40])
    return diags


def _plan(names):
    import torch
    c0 = cases.case(names[0])
    assert all((cases.case(n).plan, cases.case(n).w, cases.case(n).h, cases.case(n).intr.tobytes(), cases.case(n).wt.tobytes()) ==
               (c0.plan, c0.w, c0.h, c0.intr.tobytes(), c0.wt.tobytes()) for n in names)
    return Clouds(torch, [t for n in names for t in cases.case(n).ticks], size=c0.plan, vertex_fill=c0.fill)


def test_the_small_cases_as_ticks_of_one_plan(gpu):
    """Every 32 x 24 case from the identity and from POSE_A: mesh mode, points mode, and mesh mode again on the keys the points left."""
    small = tuple(n for n in cases.GROUPED if (cases.case(n).w, cases.case(n).h) == (cases.W, cases.H))      # (built here, not at import)
    assert len(small) >= 40 and set(cases.GROUPED) - set(small) == {"waves"}
    c = _plan(small)
    for points in (False, True, False):
        _check(c, small, points)
    c.close()


def test_more_listed_triangles_than_waves(gpu):
    c = _plan(("waves",))
    diags = _check(c, ("waves",), False)
    assert diags[0]["large"] == 240 > 2 * cases.WAVES_LAUNCHED and c.plan.capacity == 3072      # 6144 triangle slots: 24 workgroups, 96 waves
    _check(c, ("waves",), True)
    c.close()


def test_scratch_across_views_and_ticks(gpu):
    """A view that lists every triangle, one that draws nothing and a plain one take turns on the projections and the work list, in both
    orders; tick 1 is empty, tick 2 shorter than tick 0, 0x5B behind the vertices and -3 behind the triangles.  Then the plan in points
    mode, then mesh mode at a smaller view."""
    a, b = cases.case("scratch"), cases.case("scratch_reverse")
    c = _plan(("scratch",))
    diags = _check(c, ("scratch",), False)
    assert [d["large"] for d in diags] == [98, 0, 0, 0, 0, 0, 32, 0, 0] and [d["drawn"] for d in diags] == [98, 0, 98, 0, 0, 0, 32, 0, 32]
    diags = _check(c, ("scratch_reverse",), False)
    assert [d["large"] for d in diags] == [0, 98, 0, 0, 0, 0, 0, 32, 0]
    assert all(np.array_equal(x, y) for x, y in zip(a.ticks[0], b.ticks[0]))      # (the same ticks: one plan serves both)
    _check(c, ("scratch",), True)
    intr, wt, w, h = cases.SCRATCH_SMALL
    _, _, diags = c.check(intr, wt, w, h)
    assert diags[0]["pixels"] > 50 and diags[1]["pixels"] == 0 and diags[2]["pixels"] > 20
    _check(c, ("scratch",), False)
    c.close()


def test_sixteen_views_on_two_ticks(gpu):
    c = _plan(("views16",))
    diags = _check(c, ("views16",), False)
    assert len(diags) == 32 and sum(d["pixels"] > 0 for d in diags) >= 16
    _check(c, ("views16",), True)
    c.close()


def test_the_raster_grid_takes_a_second_pass(gpu):
    """512 x 257: 263168 triangle slots against 1024 workgroups of 256; the listed, the d = 1 and the out-of-range triangles lie behind
    entry 262144."""
    c = _plan(("raster_two_pass",))
    assert c.plan.capacity == 512 * 257 and 2 * c.plan.capacity > cases.RASTER_ONE_PASS
    diags = _check(c, ("raster_two_pass",), False)
    assert all(d["large"] > 100 for d in diags) and diags[1]["drawn"] == cases.RASTER_SLOTS - 40
    c.close()


def test_1024_x_1024_corner_to_corner(gpu):
    c = _plan(("budget_1024",))
    diags = _check(c, ("budget_1024",), False)
    assert diags[0]["pixels"] == 1023 * 1023 and [d["large"] for d in diags] == [2, 3]
    c.close()
