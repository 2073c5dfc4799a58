"""The boundary rigs of tests/merge_boundary_cases.py on the CPU (no GPU): a census, through merge_ref's trace, that every rig reaches the
decisions it names on both sides; the mutants of merge_ref.RULES each rig kills (a boundary that is reached but changes no output is not
covered); the closed forms against the literal loops on what the trace recorded; and merge_ref.overlay_merge against the reference's own
generateMeshFromDepthMaps(bgenerate_triangles = true) on every rig (tests/golden/merge_boundary_ref.npz, made by
tests/golden/make_merge_boundary_golden.py).

The minimum counts are conditions on the rigs, not tolerances; the measured count stands in the comment beside each."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import export_cases, merge_boundary_cases as cases, merge_ref
from tests.merge_ref import NEVER, ONE_WRITER, SEVERAL_NONE_ZERO, SMALLER_DISCARDED, ZERO_ONLY, ZERO_THEN_LATER

GOLDEN = os.path.join(export_cases.GOLDEN, "merge_boundary_ref.npz")
REFERENCE = os.environ.get("LIVESCAN3D_REFERENCE", "/root/reference")
W, H = cases.W, cases.H

_RUNS = {}


def run(orc, name, rule=None):
    """(triangles, diagnostics, trace) of merge_ref.overlay_merge on a rig, under one mutant or none; computed once."""
    if (name, rule) not in _RUNS:
        trace = {} if rule is None else None
        tris, diag = merge_ref.overlay_merge(cases.rig(name), orc, trace=trace, rules=[rule] if rule else None)
        _RUNS[name, rule] = tris, diag, trace
    return _RUNS[name, rule]


def rec(trace, kind, b, o):
    (r,) = [r for r in trace[kind] if r["b"] == b and r["o"] == o]
    return r


def class_counts(trace, b=None):
    return sum(np.bincount(d["classes"].ravel(), minlength=6) for d in trace["draw"] if b is None or d["b"] == b)


def degenerate(trace, b):
    """(den == 0 triangles, those with a box of zero area, den != 0 triangles) over the draws into base b."""
    den0 = flat = live = 0
    for d in trace["draw"]:
        if d["b"] == b and len(d["tris"]):
            s = merge_ref.triangle_setup(*d["tris"].T)
            empty = (s["maxx"] <= s["minx"]) | (s["maxy"] <= s["miny"])
            den0 += int((s["den"] == 0).sum())
            flat += int(((s["den"] == 0) & empty).sum())
            live += int((s["den"] != 0).sum())
    return den0, flat, live


# ---- census ----------------------------------------------------------------------------------------------------------------------

# name: minimum pixels of {ZERO_THEN_LATER, ZERO_ONLY} over the draws into base 1, minimum den == 0 triangles over the draws into base 0
#                        measured: (then-later, only), den == 0
ZERO_MIN = {
    "zero_m3_d1": (40, 1, 4000),      # (76, 2), 4680
    "zero_m3_d2": (10, 0, 4000),      # (20, 0), 4680
    "zero_m3_d3": (3, 0, 4000),       # (6, 0), 4680
    "zero_m2.5_d1": (25, 20, 4000),   # (50, 44), 4464
    "zero_m2.5_d2": (10, 1, 4000),    # (19, 3), 4464
    "zero_m2.5_d3": (3, 1, 4000),     # (6, 1), 4464
    "zero_roll_d3": (9, 16, 3500),    # (18, 33), 4243
}


@pytest.mark.parametrize("name", cases.ZERO_VAL)
def test_census_zero_val(orc, name):
    """Zero writers with a later writer behind them (zmax must filter, and be reset), zero writers alone (depth 0 with Z's tag), several
    writers without a zero, and -- in the minified direction -- den == 0 triangles by the thousand, some with a box of zero area and
    some without."""
    _, diag, trace = run(orc, name)
    c = class_counts(trace, b=1)
    later, only, den_min = ZERO_MIN[name]
    print(name, "classes into base 1", dict(zip(merge_ref.CLASSES, c.tolist())))
    assert c[ZERO_THEN_LATER] >= max(later, 1) and c[ZERO_ONLY] >= only, c
    assert c[NEVER] > 0 and c[ONE_WRITER] > 100 and c[SEVERAL_NONE_ZERO] > 100, c
    den0, flat, live = degenerate(trace, 0)
    print(name, "triangles into base 0: den == 0", den0, "of them with an empty box", flat, "den != 0", live)
    assert den0 >= den_min and live > 100
    # a pure scaling maps collinear points onto a row or a column alone: every box is empty; the roll with parallax leaves diagonals
    assert 0 < flat < den0 if name == "zero_roll_d3" else flat == den0, (den0, flat)
    assert class_counts(trace, b=0)[ZERO_THEN_LATER:].sum() == 0      # the true reference draws none of them
    assert diag["assigned"].sum() > 100


def test_census_zero_val_group_reaches_zero_only_often(orc):
    assert sum(class_counts(run(orc, n)[2], b=1)[ZERO_ONLY] for n in cases.ZERO_VAL) >= 50      # 83


DISCARD_MIN = {"discard_215": 2, "discard_24": 1}      # measured: 2 and 1 (and 0 / 1 ZERO_THEN_LATER pixels)


@pytest.mark.parametrize("name", sorted(DISCARD_MIN))
def test_census_discarded_smaller_val(orc, name):
    """Base 1, overlay 0: at the pixels the rig names, a writer with a non-zero val, then the last zero writer, then a larger val
    that wins; the base lies where the winner passes the depth test and the discarded writer would fail it, and the pixel
    survives the erosions -- so the merged map depends on the earlier writer being thrown away."""
    _, _, trace = run(orc, name)
    d, o = rec(trace, "draw", 1, 0), rec(trace, "overlay", 1, 0)
    pixels = cases.DISCARD_PIXELS[int(name.split("_")[1])]
    c = class_counts(trace, b=1)
    print(name, "classes into base 1", dict(zip(merge_ref.CLASSES, c.tolist())))
    assert c[SMALLER_DISCARDED] >= DISCARD_MIN[name] == len(pixels)
    k, px, py, val = merge_ref.triangle_pixels(merge_ref.triangle_setup(*d["tris"].T))
    for x, y, a, win in pixels:
        assert d["classes"][y, x] == SMALLER_DISCARDED, (x, y)
        here = (px == x) & (py == y)
        z = k[here & (val == 0)].max()
        assert val[here & (k < z) & (val != 0)].min() == a and val[here & (k > z)].min() == win, (x, y)
        p = y * W + x
        base = int(o["base_depth"][p])
        assert o["mapped"][p] == win and abs(base - win) < merge_ref.DEPTH_THRESHOLD <= abs(base - a), (x, y, base)
        assert o["tag"][p] > merge_ref.CONF_THRESHOLD and o["mask_raw"][p] and o["mask_eroded"][p], (x, y)


def test_census_all_three_zero_writer_classes_are_reached(orc):
    total = sum(class_counts(run(orc, n)[2], b=1) for n in cases.ZERO_VAL + tuple(DISCARD_MIN))
    assert (total[ZERO_THEN_LATER:] > 0).all(), total           # 196 then-later, 3 discarded, 83 zero-only


def test_census_degenerate_triangles_with_pixels(orc):
    """den0, base 0: den == 0 triangles whose box is not empty, and pixels that they alone would turn into zero writers' pixels."""
    _, _, trace = run(orc, "den0")
    den0, flat, live = degenerate(trace, 0)
    drawn = {}
    merge_ref.overlay_merge(cases.rig("den0"), orc, trace=drawn, rules=["den0_drawn"])
    a, b = rec(trace, "draw", 0, 1)["classes"], rec(drawn, "draw", 0, 1)["classes"]
    changed = int(((a < ZERO_THEN_LATER) & (b >= ZERO_THEN_LATER)).sum())
    print("den0: den == 0", den0, "with an empty box", flat, "den != 0", live, "pixels a drawn one would zero", changed)
    assert den0 - flat >= 200 and changed >= 200 and (a >= ZERO_THEN_LATER).sum() == 0


def _probe_census(o, probes):
    """[(offset, |base - mapped|, the eroded mask over the probe's 5 x 5 block)] from an "overlay" record."""
    out = []
    for (x, y), k in probes:
        p = y * W + x
        block = o["mask_eroded"].reshape(H, W)[y - 2:y + 3, x - 2:x + 3]
        assert o["tag"][p] > merge_ref.CONF_THRESHOLD and o["base_depth"][p] != 0
        out.append((k, int(abs(o["base_depth"][p] - o["mapped"][p])), block))
    return out


def test_census_depth_threshold(orc):
    """Base 0, overlay 1: every probe differs from the mapped plateau by exactly its offset, with a passing tag; 18 and 19 keep their
    5 x 5 block in the eroded mask, 20 and 21 clear it."""
    _, _, trace = run(orc, "thresholds")
    got = _probe_census(rec(trace, "overlay", 0, 1), list(zip(cases.PROBE_XY, cases.PROBE_OFFSETS)))
    assert sorted(k for k, _, _ in got) == sorted(cases.PROBE_OFFSETS)
    for k, diff, block in got:
        assert diff == abs(k), (k, diff)
        assert block.all() if abs(k) < merge_ref.DEPTH_THRESHOLD else not block.any(), k


def test_census_far(orc):
    """The same at the u16 ceiling: the plateaus come back as 65510 and 65535 and the probes sit 18 .. 21 above and below."""
    _, diag, trace = run(orc, "far")
    o = rec(trace, "overlay", 0, 1)
    assert set(np.unique(o["mapped"][o["mapped"] != 0]).tolist()) == set(cases.FAR_LEVELS) and o["base_depth"].max() == 65535
    got = _probe_census(o, cases.FAR_PROBES)
    print("far: (offset, |base - mapped|)", [(k, d) for k, d, _ in got])
    assert sorted((k, d) for k, d, _ in got) == sorted((k, abs(k)) for k in cases.PROBE_OFFSETS)
    for k, diff, block in got:
        assert block.all() if diff < merge_ref.DEPTH_THRESHOLD else not block.any(), (k, diff)


def test_census_conf_threshold(orc):
    """Base 0, overlay 1: tags 4, 5, 6 and 7 on pixels whose depth test passes, each at least 70 times (measured 144, 176, 208, 240)."""
    _, _, trace = run(orc, "confidence")
    o = rec(trace, "overlay", 0, 1)
    passes = (o["base_depth"] != 0) & (np.abs(o["base_depth"] - o["mapped"]) < merge_ref.DEPTH_THRESHOLD)
    counts = np.bincount(o["tag"][passes], minlength=21)
    print("confidence: pixels per tag", counts.tolist())
    assert (counts[4:8] >= 70).all(), counts


def test_census_shared_edges(orc):
    """Base 1 of the magnified pairs: covered pixels that lie exactly on a triangle's edge, for the edge classes the fill convention
    tells apart (DY < 0, DY > 0, DY == 0 with DX > 0, DY == 0 with DX < 0), pixels with two and with three writers, and vertices in the
    last column and row -- which stay uncovered.  The last class is there by the hundred but never covered: with the winding that
    draws at all, a horizontal edge with DX < 0 is the triangle's bottom edge, and the half-open box leaves its row out."""
    for name in ("shared_m3", "shared_m2"):
        _, _, trace = run(orc, name)
        d = rec(trace, "draw", 1, 0)
        s = merge_ref.triangle_setup(*d["tris"].T)
        k, px, py, _ = merge_ref.triangle_pixels(s)
        on = np.zeros(4, dtype=np.int64)
        for c, DX, DY in s["C"]:
            plain = c - ((DY < 0) | ((DY == 0) & (DX > 0)))
            e = (plain[k] + DX[k] * (16 * py) - DY[k] * (16 * px)) == 0
            kind = np.select([DY[k] < 0, DY[k] > 0, DX[k] > 0], [0, 1, 2], 3)
            on += np.bincount(kind[e & ((DX[k] != 0) | (DY[k] != 0))], minlength=4)
        writers = np.bincount(py * W + px, minlength=W * H)
        print(name, "edge pixels per class", on.tolist(), "pixels by writers", np.bincount(writers).tolist())
        assert (on[:3] >= 100).all() and on[3] == 0, on       # 1752, 879, 873, 0 and 2819, 1411, 1408, 0
        assert sum(int(((DY == 0) & (DX < 0)).sum()) for _, DX, DY in s["C"]) >= 100
        assert (writers == 2).sum() > 300          # 864 and 1402 (the half-open box keeps a vertex pixel from collecting more)
        m = rec(trace, "map", 1, 0)
        assert (m["x"][m["ok"]] == W - 1).sum() > 5 and (m["y"][m["ok"]] == H - 1).sum() > 5
        assert (d["classes"][:, W - 1] == NEVER).all() and (d["classes"][H - 1] == NEVER).all()
        assert (d["classes"][:, 0] == NEVER).all() and (d["classes"][0] == NEVER).all()


def test_census_project_drop(orc):
    """shift: overlay vertices at x = 0, 1, w - 1, w and y = 0, 1, h - 1, h of base 1 (kept for 1 and w - 1 / h - 1 alone) and
    triangles with exactly one dropped vertex; near_zero: vertices with d == 0 that lie inside the frame."""
    _, _, trace = run(orc, "shift")
    for (b, o), values in (((0, 1), ((0, False), (1, True))), ((1, 0), ((-1, True), (0, False)))):
        m = rec(trace, "map", b, o)
        for axis, size in (("x", W), ("y", H)):
            other, osize = ("y", H) if axis == "x" else ("x", W)
            inside = (m[other] >= 1) & (m[other] < osize)
            for v, kept in values:
                at = (m[axis] == (v if b == 0 else size + v)) & inside
                assert at.sum() >= 20 and (m["ok"][at] == kept).all(), (b, axis, v, int(at.sum()))
        t = m["tris"]
        lost = ~m["ok"][t]                                                  # per triangle and corner
        print("shift base", b, "triangles by dropped vertices", np.bincount(m["dropped"], minlength=4).tolist())
        assert (m["dropped"] == 1).sum() >= 40 and (m["dropped"] == 2).sum() >= 40 and (m["dropped"] == 0).sum() > 500   # 98 / 100 / 4640 and 101 / 103 / 890
        assert np.array_equal(lost.sum(1), m["dropped"])
    _, _, trace = run(orc, "near_zero")
    m = rec(trace, "map", 1, 0)
    inside = (m["x"] >= 1) & (m["x"] < W) & (m["y"] >= 1) & (m["y"] < H)
    print("near_zero: d == 0 inside", int(((m["d"] == 0) & inside).sum()), "d == 1", int(((m["d"] == 1) & inside).sum()),
          "one dropped", int((m["dropped"] == 1).sum()))
    assert ((m["d"] == 0) & inside).sum() >= 100 and ((m["d"] == 1) & inside).sum() >= 100        # 244 and 742; one dropped: 221
    assert not m["ok"][(m["d"] == 0)].any() and (m["dropped"] == 1).sum() >= 100


def test_census_reproject_collide(orc):
    """wobble: a sensor's own reprojection puts several vertices on one pixel, moves vertices to another pixel than their own and out of
    the frame, and gives d == 0 inside the frame."""
    _, diag, trace = run(orc, "wobble")
    for r in trace["reproject"]:
        pix = (r["y"] * W + r["x"])[r["inb"]]
        collide = len(pix) - len(np.unique(pix))
        moved = int((pix != r["v2p"][r["inb"]]).sum())
        print("wobble sensor", r["s"], "collisions", collide, "moved", moved, "left the frame", int((~r["inb"]).sum()), "d == 0 inside",
              int((r["d"][r["inb"]] == 0).sum()))
        # measured: 329 / 340 collisions, as many moved, 13 out of the frame, 1007 / 1018 with d == 0
        assert collide >= 200 and moved >= 200 and (~r["inb"]).sum() >= 5 and (r["d"][r["inb"]] == 0).sum() >= 50
    assert (diag["reprojected"] == 0).sum() > 500


def test_census_assigned_feedback(orc):
    """feedback: base 0 assigns vertices, so sensor 0 arrives at bases 1 and 2 with assigned vertices and fewer triangles; both
    overlays of every base find something, and their masks meet."""
    _, diag, trace = run(orc, "feedback")
    for b in (1, 2):
        m = rec(trace, "map", b, 0)
        assert m["assigned"].sum() >= 1000 and len(m["tris"]) < len(rec(trace, "map", 0, b)["tris"])
    first, second = [r for r in trace["overlay"] if r["b"] == 0]
    print("feedback base 0: eroded masks", int(first["mask_eroded"].sum()), int(second["mask_eroded"].sum()))
    assert first["mask_eroded"].sum() >= 300 and second["mask_eroded"].sum() >= 100      # 1160 and 1040
    assert (first["mask_eroded"] & second["mask_raw"]).sum() == 0          # what the first overlay zeroed is out of the second's mask
    grown = merge_ref.erode(merge_ref.erode((second["mask_raw"] | first["mask_eroded"]).reshape(H, W))).ravel()
    assert (grown & ~second["mask_eroded"] & ~first["mask_eroded"]).sum() > 0   # ... and that cost the second mask pixels


def test_census_tiny(orc):
    raw = {}
    for w, h in cases.TINY_SIZES:
        tris, diag, trace = run(orc, f"tiny_{w}x{h}")
        raw[w, h] = (sum(int(o["mask_raw"].sum()) for o in trace["overlay"]), sum(int(o["mask_eroded"].sum()) for o in trace["overlay"]),
                     int(diag["assigned"].sum()), len(tris))
    print("tiny: (raw mask, eroded mask, assigned, triangles)", raw)
    assert raw[2, 8] == (0, 0, 0, 0) and raw[8, 2] == (0, 0, 0, 0) and raw[8, 4] == (0, 0, 0, 0)
    assert raw[4, 8][0] >= 12 and raw[4, 8][1:3] == (0, 0) and raw[4, 8][3] > 0
    assert raw[6, 7][0] >= 24 and raw[6, 7][1:3] == (0, 0)
    assert raw[8, 9][1] >= 1 and raw[8, 9][2] >= 1


# ---- decisiveness ----------------------------------------------------------------------------------------------------------------

def _differs(a, b):
    return not (a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1]["merged"], b[1]["merged"])
                and np.array_equal(a[1]["assigned"], b[1]["assigned"]) and np.array_equal(a[1]["reprojected"], b[1]["reprojected"]))


@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.KILLS[n]])
def test_rig_kills_the_mutants_it_claims(orc, name):
    true = run(orc, name)
    for rule in cases.KILLS[name]:
        assert _differs(run(orc, name, rule), true), (name, rule)


def test_every_mutant_is_killed_by_a_named_rig(orc):
    table = {rule: [n for n in cases.NAMES if rule in cases.KILLS[n]] for rule in merge_ref.RULES}
    for rule, rigs in table.items():
        print(f"{rule:26s} {merge_ref.RULES[rule]:90s} <- {', '.join(rigs)}")
    assert all(table.values()), [r for r, rigs in table.items() if not rigs]
    assert set().union(*cases.KILLS.values()) == set(merge_ref.RULES)


def test_undecided_mutants_change_no_output(orc):
    """What merge_boundary_cases' docstring says of them, held: should one of them start to change an output, it belongs in RULES."""
    for rule in merge_ref.UNDECIDED_RULES:
        for name in cases.NAMES:
            assert not _differs(run(orc, name, rule), run(orc, name)), (rule, name)


# ---- the closed forms against the loops ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.ZERO_VAL + ("discard_215", "discard_24", "den0", "shared_m3", "near_zero", "wobble", "feedback"))
def test_draw_equals_the_sequential_loop(orc, name):
    _, _, trace = run(orc, name)
    for d in trace["draw"]:
        a = merge_ref.draw(d["tris"], d["tags"], d["w"], d["h"])
        b = merge_ref.draw_sequential(d["tris"], d["tags"], d["w"], d["h"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, d["b"], d["o"])


@pytest.mark.parametrize("name", cases.NAMES)
def test_erode_equals_the_loop(orc, name):
    _, _, trace = run(orc, name)
    for o in trace["overlay"]:
        m = o["mask_raw"].reshape(o["h"], o["w"])
        once = merge_ref.erode(m)
        assert np.array_equal(once, merge_ref.erode_loop(m))
        assert np.array_equal(merge_ref.erode(once), merge_ref.erode_loop(once))
        assert np.array_equal(merge_ref.erode(once).ravel(), o["mask_eroded"])


def test_discarded_smaller_val_on_crafted_triangles():
    """The class the discard_* rigs reach at a few pixels, with crafted triangles at many: val 2, then val 0, then val 3 on the same pixels."""
    tri = lambda d: [12, 12, d, 2, 2, d, 2, 12, d]
    tris, tags = np.array([tri(2), tri(1), tri(3)]), np.array([7, 8, 9])
    s = merge_ref.triangle_setup(*tris.T)
    k, px, py, val = merge_ref.triangle_pixels(s)
    cls = merge_ref.pixel_classes(k, py * 16 + px, val, 16 * 16)
    n = int((cls == SMALLER_DISCARDED).sum())
    assert n > 0 and (val[k == 1] == 0).any(), np.bincount(cls, minlength=6)
    a, b = merge_ref.draw(tris, tags, 16, 16), merge_ref.draw_sequential(tris, tags, 16, 16)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[0].ravel()[cls == SMALLER_DISCARDED] == 3).all() and (a[1].ravel()[cls == SMALLER_DISCARDED] == 9).all()


def test_render_ref_and_merge_ref_draw_the_same_triangles_alike(orc):
    """The two stages that share drawTriangle's arithmetic, on the CPU: the projected triangles of the magnified shared_* draws (no zero
    writer) as a mesh of their own through render_ref.render -- the same coverage and the same depths as merge_ref.draw."""
    from tests import render_ref
    intr = render_ref.intrinsics(W, H)
    for name in ("shared_m3", "shared_m2"):
        d = rec(run(orc, name)[2], "draw", 1, 0)
        assert len(d["tris"]) > 500 and (d["classes"] >= ZERO_THEN_LATER).sum() == 0
        verts, tris = render_ref.soup(d["tris"], intr)
        depth, _, info = render_ref.render(verts, tris, intr, render_ref.IDENTITY, W, H)
        want, _ = merge_ref.draw(d["tris"], d["tags"], W, H)
        assert info["drawn"] == len(tris)
        assert np.array_equal(depth != 0, d["classes"] != NEVER) and np.array_equal(depth, want), name


# ---- the reference's own code ----------------------------------------------------------------------------------------------------

def test_fixture_covers_every_rig():
    z = np.load(GOLDEN)
    assert tuple(str(n) for n in z["names"]) == cases.NAMES
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(export_cases.GOLDEN, "export_ref.npz"))


@pytest.mark.parametrize("name", cases.NAMES)
def test_merge_ref_equals_reference_fixture(orc, name):
    z = np.load(GOLDEN)
    rig = cases.rig(name)
    assert str(z[name + "/inputs"]) == export_cases.sha(export_cases.rig_inputs(rig)), "the rig is no longer the one the fixture was made from"
    tris, diag, _ = run(orc, name)
    assert cases.equals_fixture(z, name, tris)
    assert int(z[name + "/n_vertices"]) == int(diag["offsets"][-1]) and np.array_equal(z[name + "/offsets"], diag["offsets"])


def test_generator_reproduces_the_fixture(tmp_path):
    """Reruns the reference on every rig where a checkout is present (the only test here that reads it): byte-identical arrays."""
    if not os.path.exists(os.path.join(REFERENCE, "src", "NativeUtils", "depthprocessing.cpp")):
        pytest.skip("no LiveScan3D checkout at $LIVESCAN3D_REFERENCE; the committed fixture stands for it")
    gen = os.path.join(export_cases.GOLDEN, "make_merge_boundary_golden.py")
    subprocess.check_call([sys.executable, gen, REFERENCE, str(tmp_path)], stdout=subprocess.DEVNULL, timeout=600)
    fresh, z = np.load(tmp_path / "merge_boundary_ref.npz"), np.load(GOLDEN)
    assert sorted(fresh.files) == sorted(z.files)
    for k in z.files:
        assert fresh[k].dtype == z[k].dtype and fresh[k].tobytes() == z[k].tobytes(), k
