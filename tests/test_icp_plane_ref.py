"""The point-to-plane ICP step's definition (tests/icp_plane_ref.py) and its cases (tests/icp_plane_cases.py), on the CPU.

Every case is built once with its witness (`_check_case`) and its regime conditions; the mutants of the definition are each killed by a
named case, by more than a hundred times the tolerance `bounds` grants an implementation; a second, independent statement of the step
(least squares on the stacked rows of J) agrees with `step`; and the definition's shared parts are icp_step_ref's own objects."""
import numpy as np
import pytest

from tests import icp_plane_cases as cases
from tests import icp_plane_ref as pref
from tests import icp_step_ref as ref

F32 = np.float32


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_reaches_what_it_is_named_for(orc, name):
    c = cases.get(name, orc)
    s = c.step0
    assert s["mk"] <= s["n_kept"] <= s["m"] <= min(len(c.tgt), len(c.src))
    b = pref.bounds(s)
    assert np.isfinite(b["T"]).all() and np.isfinite(b["Rn"]).all()
    if s["mk"] > 0 and s["kept_modes"].any():
        # the tolerances are a few f32 ulps of a motion of centimetres and degrees: the double sums never dominate them
        assert b["dx"] < 1e-9 and (b["Rn"] <= 2.0 ** -22).all() and (b["T"] <= 1e-6).all(), b


def test_corner_converges_where_point_to_point_creeps(orc):
    start, plane, point = cases.get("corner", orc).extra["chain_distances"]
    print(f"corner: mean wall distance {start:.3e} m -> {plane:.3e} m after 3 plane iterations, {point:.3e} m after 10 point-to-point iterations")
    assert 100 * plane <= point < start


def test_shared_parts_are_the_point_to_point_definitions(orc):
    assert pref.apply32 is ref.apply32 and pref.compose32 is ref.compose32 and pref.winners is ref.winners
    for name in ("chain", "zero_normals", "block_edges_257"):
        c = cases.get(name, orc)
        s, p = c.step0, ref.step(c.tgt, c.src, c.idx, c.d2)
        assert np.array_equal(s["winners"], p["winners"]) and np.array_equal(s["keep"], p["keep"])
        assert (s["m"], s["n_kept"], s["mean"], s["sd"], s["margin"]) == (p["m"], p["mk"], p["mean"], p["sd"], p["margin"])


MUTANTS = {
    # the wrong variant: (arguments of step that select it, the case that kills it)
    "wrong sign of g": (dict(g_sign=+1.0), "corner"),
    "a x n instead of b x n": (dict(cross_of="a"), "corner"),
    "Rn = Rinc instead of its transpose": (dict(rn_transposed=False), "corner"),
    "T = tau": (dict(t_rotated=False), "far_from_origin"),
    "a cutoff at 0": (dict(cutoff=0.0), "single_wall"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_of_the_definition_is_killed(orc, mutant):
    kwargs, name = MUTANTS[mutant]
    c = cases.get(name, orc)
    wrong = pref.step(c.tgt, c.nrm, c.src, c.idx, c.d2, **kwargs)
    far = cases.killed(c.step0, wrong)
    print(f"{mutant}: {far:.3g} tolerances away on {name}")
    assert far > 100, (mutant, name, far)


@pytest.mark.parametrize("name", cases.FULL_RANK)
def test_least_squares_on_the_stacked_rows_agrees(orc, name):
    """A x = -g is the normal equation of min |J x + r|: numpy's SVD-based least squares on the rows themselves, with the cutoff restated
    for singular values (sigma^2 = lambda), must give the same step."""
    c = cases.get(name, orc)
    s = c.step0
    assert s["kept_modes"].all()
    x, _, rank, sv = np.linalg.lstsq(s["J"], -s["r"], rcond=np.sqrt(pref.CUTOFF))
    assert rank == 6 and np.allclose(np.sort(sv ** 2), s["lam"], rtol=1e-9)
    err = np.abs(x - s["x"]).max() / np.abs(x).max()
    print(f"{name}: lstsq vs step {err:.2e}")
    assert err <= 1e-12


def test_rodrigues_and_motion_form():
    rng = np.random.default_rng(3)
    assert np.array_equal(pref.rodrigues(np.zeros(3)), np.eye(3))
    for scale in (1e-9, 0.9 * pref.SERIES_BELOW, 1.1 * pref.SERIES_BELOW, 0.07, 2.0):
        w = rng.normal(size=3)
        w *= scale / np.linalg.norm(w)
        R = pref.rodrigues(w)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert np.abs(R @ w - w).max() < 1e-16 * max(scale, 1) and abs(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)) - scale) < 1e-8
        # the library's row-vector form v' = (v + T) Rn is the column form Rinc v + tau
        tau, v = rng.normal(size=3), rng.normal(size=3)
        T, Rn = pref.motion(np.concatenate([w, tau]))
        assert np.abs((v + T) @ Rn - (R @ v + tau)).max() < 1e-15


def test_usable_is_the_f32_rule():
    tiny = F32(1e-23)                                           # its square underflows to zero in f32, not in double
    n = np.array([[0, 0, 0], [0, 0, 1], [np.nan, 0, 1], [0, np.inf, 0], [tiny, 0, 0], [-0.0, 0, -2], [3e38, 3e38, 0]], F32)
    assert pref.usable(n).tolist() == [False, True, False, False, False, True, True]
