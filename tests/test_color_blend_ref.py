"""The colour blend's definition (tests/color_blend_ref.py, numpy) on the hand-made rigs of tests/color_blend_cases.py, without a GPU:
held bit for bit to the plain-Python triple loop (tests/color_blend_ref_py.py), every case to its witness -- what it is named for is
reached, read from the definition alone -- and to the mutants it is listed to kill.  Suite conditions: every case that is not named a
no-op changes at least one vertex, the no-ops none; every mutant of color_blend_ref_py.RULES is killed by some case; alpha, X, Y, Z of
every vertex survive everywhere."""
import numpy as np
import pytest

from tests import color_blend_cases as cases, color_blend_ref as ref, color_blend_ref_py as ref_py, color_ref

INT_MIN = -2 ** 31
_results = {}


def _result(orc, name):
    """Per tick of a case: (the cloud handed in, the definition's output, its diagnostics, its terms).  Computed once, never changed."""
    if name not in _results:
        c, out = cases.case(name), []
        for k, rig in enumerate(c.ticks):
            v0, terms = cases.start(c, k, orc), []
            v, d = ref.blend(rig, orc, c.tol, c.minc, verts=v0, terms=terms)
            for a in (v0, v, *d.values()):
                a.setflags(write=False)
            out.append((v0, v, d, terms))
        _results[name] = out
    return _results[name]


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(np.array_equal(a[1][k], b[1][k]) for k in ("blended", "partners", "abs_change"))


def _loops(orc, name, rules=()):
    c = cases.case(name)
    return ref_py.blend_ticks(c.ticks, orc, c.tol, c.minc, verts=[cases.start(c, k, orc) for k in range(len(c.ticks))], rules=rules)


@pytest.mark.parametrize("name", cases.NAMES)
def test_numpy_equals_the_python_loops(orc, name):
    for k, ((v0, v, d, _), got) in enumerate(zip(_result(orc, name), _loops(orc, name))):
        assert _same((v, d), got), (name, k)


@pytest.mark.parametrize("name", cases.NAMES)
def test_only_the_colour_bytes_change_and_only_where_named(orc, name):
    c = cases.case(name)
    changed = 0
    for v0, v, d, _ in _result(orc, name):
        a, b = v0.view(np.uint8).reshape(-1, 16), v.view(np.uint8).reshape(-1, 16)
        assert a[:, 3:].tobytes() == b[:, 3:].tobytes(), name      # alpha and the bits of X, Y, Z
        changed += int((a[:, :3] != b[:, :3]).any(axis=1).sum())
        assert int(d["abs_change"].sum()) == int(np.abs(a[:, :3].astype(int) - b[:, :3].astype(int)).sum())
    assert (changed == 0) == c.noop, (name, changed)


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.case(n).kills])
def test_the_listed_mutants_are_killed(orc, name):
    right = [(v, d) for _, v, d, _ in _result(orc, name)]
    for rule in cases.case(name).kills:
        wrong = _loops(orc, name, rules=(rule,))
        assert not all(_same(a, b) for a, b in zip(right, wrong)), (name, rule, ref_py.RULES[rule])


def test_every_mutant_is_killed_by_some_case():
    killed = {r for n in cases.NAMES for r in cases.case(n).kills}
    assert killed == set(ref_py.RULES), set(ref_py.RULES) ^ killed


def test_33_sensors_are_refused(orc):
    with pytest.raises(ref.Refused, match="at most 32 sensors"):
        ref.blend(cases.rig33(), orc, 15, 1)
    with pytest.raises(ValueError, match="at most 32 sensors"):
        ref_py.blend_ticks([cases.rig33()], orc, 15, 1)


# ---- witnesses: what every case reaches, read from the definition's own terms ----------------------------------------------------------

def _pairs(terms):
    return [t for t in terms if t["i"] is not None]


def _sums(terms, j):
    return next(t for t in terms if t["i"] is None and t["j"] == j)


def _cat(terms, key):
    return np.concatenate([t[key] for t in _pairs(terms)])


def _w_rounding(orc, c, res):
    hit = set()
    for j in (0, 1):
        s = _sums(res[0][3], j)
        W, num = s["W"][s["has"]], s["num"][s["has"]]
        r = (num + (W // 2)[:, None]) % W[:, None]
        assert (W > 20).all() and len({int(w) for w in W}) >= 5      # 20 + 1 .. 4 and 20 + 20
        hit |= {"on"} if (r == 0).any() else set()
        hit |= {"below"} if (r == W[:, None] - 1).any() else set()
        hit |= {"above"} if (r == 1).any() else set()
        assert ((W % 2 == 1)[:, None] & (r == W[:, None] - 1)).any()      # an odd W one below: floor(W / 2) and ceil(W / 2) part here
    assert hit == {"on", "below", "above"}


def _w_tol_edge(orc, c, res):
    t = res[0][3]
    diff, took, inside = _cat(t, "d1") - _cat(t, "d2"), _cat(t, "took_part"), _cat(t, "inside")
    for d, want in ((c.tol - 1, True), (-(c.tol - 1), True), (c.tol, False), (-c.tol, False)):
        at = inside & (diff == d)
        assert at.any() and (took[at] == want).all(), d


def _w_conf_edge(orc, c, res):
    t = next(t for t in _pairs(res[0][3]) if (t["j"], t["i"]) == (0, 1))
    for w, want in ((c.minc - 1, False), (c.minc, True)):
        at = t["inside"] & (t["w"] == w) & (t["d2"] > 0)
        assert at.any() and (t["took_part"][at] == want).all(), w
    own = _sums(res[0][3], 1)
    assert (own["has"] & (own["own"] == 1)).any()      # the own term at confidence 1, below min_confidence


def _w_crop_hole(orc, c, res):
    S = ref.sensors_of(c.ticks[0], orc)
    assert len(S[0].verts) == cases.CROP_KEPT and len(S[1].verts) == 48
    t = next(t for t in _pairs(res[0][3]) if (t["j"], t["i"]) == (1, 0))
    no_vertex = t["inside"] & (t["d2"] > 0) & (np.abs(t["d1"] - t["d2"]) < c.tol) & (t["w"] >= 1) & (t["v"] < 0)
    assert int(no_vertex.sum()) == 48 - cases.CROP_KEPT and int(t["took_part"].sum()) == cases.CROP_KEPT


def _w_proj_shift(orc, c, res):
    t = res[0][3]
    assert {-1, 0, 15, 16} <= set(_cat(t, "x").tolist()) and {-1, 0, 11, 12} <= set(_cat(t, "y").tolist())


def _w_behind(orc, c, res):
    t = next(t for t in _pairs(res[0][3]) if (t["j"], t["i"]) == (1, 0))
    only_d1 = t["inside"] & (t["d1"] == 0) & (t["d2"] > 0) & (np.abs(t["d1"] - t["d2"]) < c.tol) & (t["v"] >= 0) & (t["w"] >= 1)
    assert only_d1.sum() > 50 and not t["took_part"][only_d1].any() and t["took_part"].sum() > 50


def _w_far(orc, c, res):
    t = next(t for t in _pairs(res[0][3]) if (t["j"], t["i"]) == (1, 0))
    assert (t["took_part"] & (t["d1"] == 65535)).sum() > 1000


def _w_nan_pose(orc, c, res):
    for t in _pairs(res[0][3]):
        if 1 in (t["j"], t["i"]):
            assert (t["x"] == INT_MIN).all() and not t["took_part"].any()
    assert res[0][2]["blended"].tolist() == [48, 0, 48]


def _w_three(orc, c, res):
    v = res[0][1]
    want = [(20 * sum(col[ch] for col in cases.THREE_COLORS) + 30) // 60 for ch in range(3)]
    assert len(v) == 3 * 48 and all((v[k] == want[q]).all() for q, k in enumerate("RGB"))
    assert res[0][2]["partners"].tolist() == [96, 96, 96]


def _w_jacobi(orc, c, res):
    """An in-place sweep, sensor by sensor, built from the definition alone: sensor 0 blended from the colours handed in, then sensor 1
    from a cloud in which sensor 0 already carries its new colours.  Sensor 1's bytes differ from the true (Jacobi) ones."""
    v0, v, d, _ = res[0]
    assert d["blended"].min() > 100 and len(np.unique(v["R"])) > 10
    _, off = ref.fused(ref.sensors_of(c.ticks[0], orc))
    swept = np.array(v0, copy=True)
    swept[:off[1]] = v[:off[1]]
    second = ref.blend(c.ticks[0], orc, c.tol, c.minc, verts=swept)[0]
    assert second[off[1]:].tobytes() != v[off[1]:].tobytes()


def _w_after_transfer(orc, c, res):
    plain, _ = ref.fused(ref.sensors_of(c.ticks[0], orc))
    moved = color_ref.color_transfer(c.ticks[0], orc)
    assert moved[1]["pairs"] and res[0][0].tobytes() == moved[0].tobytes() != plain.tobytes()


def _w_size(orc, c, res):
    S = ref.sensors_of(c.ticks[0], orc)
    w, h = S[0].w, S[0].h
    assert res[0][2]["blended"].min() >= max(1, w * h - 2)
    if w >= 33:
        conf = S[0].conf.reshape(h, w)
        assert conf[h // 2, 29] < 20 and conf[h // 2, 32] < 20 and conf.max() == 20 and conf[h - 3, w - 3] == 1


def _w_mixed(orc, c, res):
    assert len(set(c.ticks[0].widths.tolist())) == 3 and res[0][2]["blended"].min() >= 4


def _w_count(total):
    def w(orc, c, res):
        _, off = ref.fused(ref.sensors_of(c.ticks[0], orc))
        assert off.tolist() == [0, 100, total] and res[0][2]["blended"].min() > 50
    return w


def _w_two_ticks(orc, c, res):
    a, b = (ref.sensors_of(r, orc) for r in c.ticks)
    assert any(not np.array_equal(x.conf, y.conf) for x, y in zip(a, b)) and res[0][1].tobytes() != res[1][1].tobytes()
    assert len(res[0][1]) != len(res[1][1])      # other holes: other pixel -> vertex maps


def _w_n32(orc, c, res):
    top = max(int(t["num"].max()) for t in res[0][3] if t["i"] is None)
    assert top == 32 * 20 * 255 and res[0][2]["partners"].tolist() == [16 * 31] * 32


def _w_min_conf0(orc, c, res):
    as_one = ref.blend(c.ticks[0], orc, c.tol, 1)
    assert _same((res[0][1], res[0][2]), as_one) and res[0][2]["blended"].sum() > 0


def _w_alpha(orc, c, res):
    a = res[0][0]["A"]
    assert a[0] == 0 and a[1] == 255 and len(set(a.tolist())) > 20 and np.array_equal(res[0][1]["A"], a)


def _w_noop(orc, c, res):
    assert all(not d["blended"].any() and not d["partners"].any() for _, _, d, _ in res)


WITNESS = {
    "one_sensor": _w_noop, "no_overlap": _w_noop, "off_tol0": _w_noop, "off_conf21": _w_noop,
    "rounding": _w_rounding, "tol_edge": _w_tol_edge, "conf_edge": _w_conf_edge, "crop_hole": _w_crop_hole, "proj_shift": _w_proj_shift,
    "behind": _w_behind, "far": _w_far, "nan_pose": _w_nan_pose, "three": _w_three, "jacobi": _w_jacobi, "after_transfer": _w_after_transfer,
    **{f"size_{w}x{h}": _w_size for w, h in cases.SIZES}, "mixed": _w_mixed,
    **{f"count_{t}": _w_count(t) for t in (255, 256, 257)},
    "two_ticks": _w_two_ticks, "n32": _w_n32, "min_conf0": _w_min_conf0, "alpha": _w_alpha,
}


@pytest.mark.parametrize("name", cases.NAMES)
def test_witness(orc, name):
    assert set(WITNESS) == set(cases.NAMES)
    WITNESS[name](orc, cases.case(name), _result(orc, name))
