"""The boundary rigs of tests/color_boundary_cases.py on the CPU (no GPU).

Reach: a census, through the restatements' own intermediate values, that every rig reaches the decision it names -- the exact coverage,
the exact number of samples, samples with d1 == 0, columns that project into (-1, 0), the confidence values on either side of a pair,
the corridor's levels, the pair list (test_reach_*).
Sensitivity: for every rig the mutants of color_ref_py.RULES it claims (color_boundary_cases.KILLS) -- the neighbouring wrong rule at
one decision -- change the output bytes or the diagnostics, and every mutant is killed by a named rig (test_rig_kills_*,
test_every_mutant_*): a boundary that is reached but decides nothing is not covered.
Agreement: color_ref.color_transfer equals color_ref_py.color_transfer on every rig.
Reference: color_ref equals the reference's own generateMeshFromDepthMaps(bcolor_transfer = true) on every rig outside DEFINED
(tests/golden/color_boundary_ref.npz, made by tests/golden/make_color_boundary_golden.py).

The counts asserted are conditions on the rigs, not tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import color_boundary_cases as cases, color_ref, color_ref_py, export_cases

GOLDEN = os.path.join(export_cases.GOLDEN, "color_boundary_ref.npz")
REFERENCE = os.environ.get("LIVESCAN3D_REFERENCE", "/root/reference")
W, H = cases.W, cases.H

_REF, _PY, _SENSORS = {}, {}, {}


def ref(orc, name):
    if name not in _REF:
        _REF[name] = color_ref.color_transfer(cases.rig(name), orc)
    return _REF[name]


def py(orc, name, rule=None):
    if (name, rule) not in _PY:
        _PY[name, rule] = color_ref_py.color_transfer(cases.rig(name), orc, rules=[rule] if rule else ())
    return _PY[name, rule]


def same(a, b):
    """Two (vertices, diagnostics) results: (the bytes are equal, the diagnostics are equal)."""
    (va, da), (vb, db) = a, b
    return va.tobytes() == vb.tobytes(), (np.array_equal(da["confidence"], db["confidence"]) and np.array_equal(da["coverage"], db["coverage"])
                                          and [tuple(p) for p in da["pairs"]] == [tuple(p) for p in db["pairs"]]
                                          and np.asarray(da["transforms"]).tobytes() == np.asarray(db["transforms"]).tobytes())


def sensors(orc, name):
    if name not in _SENSORS:
        r = cases.rig(name)
        po = [0] + np.cumsum(r.widths.astype(np.int64) * r.heights).tolist()
        _SENSORS[name] = [color_ref.Sensor(d, r.depth_colors[3 * po[k]:3 * po[k + 1]].reshape(d.shape + (3,)), r.intr[7 * k:7 * k + 7],
                                           r.wt[12 * k:12 * k + 12], r.bounds, orc) for k, d in enumerate(cases.frames(r))]
    return _SENSORS[name]


def decisions(orc, name, i, j):
    """What decides about sensor j's vertices in sensor i: the projection, both confidences, both masks, the vertex of the pixel."""
    s = sensors(orc, name)
    x, y, d1 = color_ref.project(s[j].verts["X"], s[j].verts["Y"], s[j].verts["Z"], s[i].intr, s[i].wt)
    cov, q = color_ref._tests(s[i], s[j], True)
    smp, _ = color_ref._tests(s[i], s[j], False)
    inb = (x >= 0) & (x < s[i].w) & (y >= 0) & (y < s[i].h)
    return dict(x=x, y=y, d1=d1, inb=inb, q=q, cov=cov, smp=smp, gi=s[i].p2v[q], conf_i=np.where(inb, s[i].conf[q], -1),
                conf_j=s[j].conf[s[j].v2p], d2=np.where(inb, s[i].depth.ravel()[q].astype(np.int64), -1))


def conf_maps(orc, name):
    r = cases.rig(name)
    c, out, po = ref(orc, name)[1]["confidence"], [], 0
    for w, h in zip(r.widths.tolist(), r.heights.tolist()):
        out.append(c[po:po + w * h].reshape(h, w).astype(np.int64))
        po += w * h
    return out


# ---- reach -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(100, 109))
def test_reach_coverage_threshold_and_fold_tail(orc, k):
    """Coverage exactly k: 100 chooses nothing, 101 .. 108 choose (0, 1) with exactly k samples, none of them skipped."""
    name = f"cov_{k}"
    v, d = ref(orc, name)
    t = decisions(orc, name, 0, 1)
    assert d["coverage"][0, 1] == k == t["cov"].sum() and (d["confidence"] == 20).all()
    assert d["pairs"] == ([] if k == 100 else [(0, 1)])
    assert (t["smp"] & (t["gi"] >= 0)).sum() == k and name not in cases.DEFINED
    plain = np.concatenate([s.verts for s in sensors(orc, name)])
    assert (v.tobytes() == plain.tobytes()) == (k == 100)
    assert sorted(int(n.split("_")[1]) % 8 for n in cases.TAIL) == list(range(8))


@pytest.mark.parametrize("k", cases.NS)
def test_reach_small_sample_counts(orc, k):
    """ns_K: the coverage is the whole frame, (0, 1) is chosen, 3072 - K samples have depth and no vertex, exactly K survive."""
    name = f"ns_{k}"
    v, d = ref(orc, name)
    t = decisions(orc, name, 0, 1)
    assert d["coverage"][0, 1] == W * H and d["pairs"] == [(0, 1)] and name in cases.DEFINED
    assert (t["smp"] & (t["gi"] >= 0)).sum() == k and (t["smp"] & (t["gi"] < 0)).sum() == W * H - k
    if k == 0:
        assert d["transforms"].tolist() == [[0.0] * 6 + [1.0] * 3]
        assert v.tobytes() == np.concatenate([s.verts for s in sensors(orc, name)]).tobytes()


def test_reach_depth_steps_between_sensors(orc):
    _, d = ref(orc, "between")
    assert d["coverage"][0, 1] == d["coverage"][0, 2] == W * H // 2 and d["coverage"][1, 2] == 0 and d["pairs"] == [(0, 1), (0, 2)]
    for j, sign in ((1, 1), (2, -1)):
        t = decisions(orc, "between", 0, j)
        assert t["inb"].all() and (t["conf_i"] == 20).all() and (t["conf_j"] == 20).all()
        for step in cases.BETWEEN_STEPS:
            at = (t["d1"] - t["d2"]) == sign * step
            assert at.sum() == W * H // 4 and (t["cov"][at] == (step < 20)).all() and (t["smp"][at] == (step < 20)).all(), (j, step)


def test_reach_depth_steps_inside_a_frame(orc):
    """frame_steps: every block lies beside pixels the BFS reached early; it enters the blocks 19 off and not those 20 off.
    seed_steps: a pixel 21 off seeds itself and both neighbours on its diagonal, a pixel 20 off seeds nothing."""
    c = conf_maps(orc, "frame_steps")[0]
    hx, hy = cases.STEP_HOLE
    assert c[hy, hx] == 0 and c[hy - 1, hx - 1] == 1 and c[hy + 1, hx + 1] == 1
    for k, (x, y) in cases.STEP_BLOCKS.items():
        block, ring = c[y:y + 2, x:x + 2], c[y - 1:y + 3, x - 1:x + 3]
        assert ring.min() <= 4, (k, ring)
        assert (block == 20).all() if abs(k) == 20 else ((block >= 2) & (block <= 5)).all(), (k, block)
    c = conf_maps(orc, "seed_steps")[0]
    for k, (x, y) in cases.SEED_PROBES.items():
        if abs(k) == 21:
            assert c[y, x] == c[y - 1, x - 1] == c[y + 1, x + 1] == 1 and c[y - 1, x] == 2, k
        else:
            assert (c[y - 3:y + 4, x - 3:x + 4] == 20).all(), k


@pytest.mark.parametrize("name", ("conf_i", "conf_j"))
def test_reach_confidence_on_one_side(orc, name):
    """The ramp lies on one side of the pair alone: 4 is refused and 5 accepted there while the other side is 20 everywhere."""
    t = decisions(orc, name, 0, 1)
    mine, other = ("conf_i", "conf_j") if name == "conf_i" else ("conf_j", "conf_i")
    assert (t[other] == 20).all() and t["inb"].all()
    counts = np.bincount(t[mine], minlength=21)
    assert counts[4] >= 20 and counts[5] >= 20, counts           # 32 and 40
    assert not t["cov"][t[mine] == 4].any() and t["cov"][t[mine] == 5].all() and not t["smp"][t[mine] == 4].any() and t["smp"][t[mine] == 5].all()
    assert ref(orc, name)[1]["pairs"] == [(0, 1)]


def test_reach_corridor(orc):
    """Every corridor pixel's level is 1 + its distance from the seed ALONG the corridor, capped at 20; nothing beside the corridor is
    within 20 of it; the walk crosses x = 32 and y = 32, and the pixels with 19 and 20 lie in another 32 x 32 tile than the seed."""
    d = cases.frames(cases.rig("corridor"))[0].astype(np.int64)
    c = conf_maps(orc, "corridor")[0]
    path = cases.corridor_path()
    on = set(path)
    assert len(path) - 1 >= 19 and path[0] == cases.CORRIDOR_START and c[path[0][1], path[0][0]] == 1
    dist = {path[0]: 0}
    todo = [path[0]]
    while todo:
        x, y = todo.pop(0)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                p = (x + dx, y + dy)
                if p in on and p not in dist:
                    dist[p] = dist[x, y] + 1
                    todo.append(p)
                elif p not in on and (dx or dy) and p != (path[0][0] - 1, path[0][1] - 1):
                    assert abs(d[p[1], p[0]] - d[y, x]) >= 20, p
    levels = [int(c[y, x]) for x, y in path]
    assert levels == [min(1 + dist[p], 20) for p in path]
    assert set(range(1, 21)) <= set(levels)
    x19, y19 = path[levels.index(19)]
    assert path[0][0] < 32 and path[0][1] < 32 and x19 >= 32 and y19 >= 32 and levels[-1] == 20
    assert {x for x, _ in path} >= {31, 32} and {y for _, y in path} >= {31, 32}


@pytest.mark.parametrize("w,h", cases.SIZES)
def test_reach_frame_edges(orc, w, h):
    name = f"size_{w}x{h}"
    d, c = cases.frames(cases.rig(name))[0], conf_maps(orc, name)[0]
    assert d.shape == (h, w) and (d[h - 1] != 0).any() and (d[:, w - 1] != 0).any()
    assert (c[0] == 20).all() and (c[:, 0] == 20).all()            # never visited, never a seed
    if min(w, h) < 3:
        assert (c == 20).all()
        return
    assert c[1, 1] == 1 and c[h - 2, w - 2] == 1                     # seeds beside the first and the last row and column
    assert (c[h - 1] == 2).any() and (c[:, w - 1] == 2).any() and c[h - 1, w - 2] == 2 and c[h - 2, w - 1] == 2
    if w >= 5:
        assert d[0, 1] != 0 and d[1, 0] != 0 and c[0, 1] == 20 and c[1, 0] == 20     # reachable but for the border rule


def test_reach_projection_edges(orc):
    r = cases.rig("proj_frac")
    rx, ry, _ = cases.raw_projection(r, 0, 1, orc)
    t = decisions(orc, "proj_frac", 0, 1)
    neg_x, neg_y = (rx > -1) & (rx < 0), (ry > -1) & (ry < 0)
    assert neg_x.sum() == H and neg_y.sum() == W and (t["x"][neg_x] == 0).all() and (t["y"][neg_y] == 0).all()
    assert t["cov"][neg_x | neg_y].all() and ref(orc, "proj_frac")[1]["coverage"][0, 1] == W * H
    t = decisions(orc, "proj_over", 0, 1)
    assert (t["x"] == W).sum() == H and (t["y"] == H).sum() == W and t["x"].max() == W and t["y"].max() == H
    assert not t["inb"][(t["x"] == W) | (t["y"] == H)].any() and ref(orc, "proj_over")[1]["coverage"][0, 1] == (W - 1) * (H - 1)
    t = decisions(orc, "proj_frame", 0, 1)
    assert (t["x"] == W - 1).sum() == H and (t["x"] == W).sum() == H and t["inb"].sum() == H
    assert ref(orc, "proj_frame")[1]["coverage"][0, 1] == H and ref(orc, "proj_frame")[1]["pairs"] == []


def test_reach_depth_clamp(orc):
    _, _, tz = cases.raw_projection(cases.rig("far"), 0, 1, orc)
    t = decisions(orc, "far", 0, 1)
    assert (tz * np.float32(1000.0) > 65999).all() and (t["d1"] == 65535).all() and t["cov"][t["inb"]].all()
    assert ref(orc, "far")[1]["pairs"] == [(0, 1)]


def test_reach_d1_zero_samples(orc):
    """d1zero: vertices behind sensor 0 (tz < 0) project mirrored into its frame with d1 == 0; the coverage refuses them all, the sample
    pass takes those that land on the 10 mm patch; the block carries the coverage."""
    _, _, tz = cases.raw_projection(cases.rig("d1zero"), 0, 1, orc)
    t = decisions(orc, "d1zero", 0, 1)
    back = tz < 0
    assert back.sum() > 5000 and (t["d1"][back] == 0).all() and (t["inb"] & back).sum() > 1000
    zero = t["smp"] & (t["d1"] == 0)
    assert zero.sum() >= 1000 and not t["cov"][zero].any() and (t["d2"][zero] == 10).all() and (t["gi"][zero] >= 0).all()    # 2541
    _, d = ref(orc, "d1zero")
    assert d["coverage"][0, 1] == t["cov"].sum() == 900 and d["pairs"] == [(0, 1)] and t["smp"].sum() == 900 + zero.sum()


def test_reach_camera_plane(orc):
    """plane: tz == 0 exactly; x and y are infinite or (on the principal row and column) NaN, and INT_MIN after the conversion."""
    rx, ry, tz = cases.raw_projection(cases.rig("plane"), 0, 1, orc)
    t = decisions(orc, "plane", 0, 1)
    flat = tz == 0
    assert flat.sum() > 5000 and (np.isnan(rx) & flat).sum() >= 50 and (np.isnan(ry) & flat).sum() >= 50 and (np.isnan(rx) & np.isnan(ry)).sum() == 1
    assert (np.isinf(rx) & flat).sum() > 5000 and (t["x"][flat] == color_ref.INT_MIN).all() and (t["y"][flat] == color_ref.INT_MIN).all()
    assert not t["inb"][flat].any() and ref(orc, "plane")[1]["coverage"][0, 1] == 900
    s0 = sensors(orc, "plane")[0]
    assert s0.depth[0, 0] == 10 and s0.conf[0] == 20 and s0.p2v[0] == 0      # where a NaN turned into 0 would find a sample


PAIRS = {
    "tie_first": ([(0, 1), (0, 2), (0, 3)], {(0, 1): 3072, (0, 2): 150, (0, 3): 150, (1, 2): 150, (1, 3): 150, (2, 3): 150}),
    "tie_second": ([(0, 1), (0, 2), (2, 3)], {(0, 1): 3072, (0, 2): 150, (0, 3): 150, (1, 2): 150, (1, 3): 150, (2, 3): 3072}),
    "b1_gt_b2": ([(2, 3), (2, 0), (0, 1)], {(0, 2): 500, (0, 3): 490, (1, 2): 500, (1, 3): 500, (2, 3): 3062}),
    "early_end": ([(0, 1)], {(0, 1): 3072, (0, 2): 50, (0, 3): 50, (1, 2): 50, (1, 3): 50, (2, 3): 2860}),
}


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_reach_pairing(orc, name):
    _, d = ref(orc, name)
    pairs, table = PAIRS[name]
    assert d["pairs"] == pairs
    for (i, j), c in table.items():
        assert d["coverage"][i, j] == d["coverage"][j, i] == c, (i, j)
    if name == "b1_gt_b2":
        assert d["coverage"][0, 1] < d["coverage"][2, 3] and any(a > b for a, b in d["pairs"])


def test_reach_32_sensors(orc):
    _, d = ref(orc, "n32")
    c = d["coverage"]
    assert c.shape == (32, 32) and (c[~np.eye(32, dtype=bool)] > 100).all() and len(d["pairs"]) == 31
    assert sorted(j for _, j in d["pairs"]) == sorted(set(range(32)) - {d["pairs"][0][0]})       # every other sensor is corrected once
    assert any(31 in p for p in d["pairs"][:-1]) and any(a > b for a, b in d["pairs"])


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in cases.NAMES if cases.KILLS[n]])
def test_rig_kills_the_mutants_it_claims(orc, name):
    true = py(orc, name)
    for rule in cases.KILLS[name]:
        bytes_same, diag_same = same(py(orc, name, rule), true)
        print(f"{name:12s} {rule:28s} bytes {'same' if bytes_same else 'differ'}, diagnostics {'same' if diag_same else 'differ'}")
        assert not (bytes_same and diag_same), (name, rule)


def test_every_mutant_is_killed_by_a_named_rig():
    table = {rule: [n for n in cases.NAMES if rule in cases.KILLS[n]] for rule in color_ref_py.RULES}
    for rule, rigs in table.items():
        print(f"{rule:28s} {color_ref_py.RULES[rule]:80s} <- {', '.join(rigs)}")
    assert all(table.values()), [r for r, rigs in table.items() if not rigs]
    assert set().union(*cases.KILLS.values()) == set(color_ref_py.RULES) and set(cases.KILLS) == set(cases.NAMES)


def test_the_two_confidence_tests_are_told_apart(orc):
    """A wrong threshold on one side changes the rig whose ramp lies on that side, and not the other rig."""
    for name, other in (("conf_i", "conf_j"), ("conf_j", "conf_i")):
        for k in (4, 6):
            assert same(py(orc, name, f"{other}_ge_{k}"), py(orc, name)) == (True, True), (name, other, k)


def test_the_two_d1_tests_are_told_apart(orc):
    """d1zero: a d1 test in the sample pass changes the transform (and bytes); none in the coverage changes the table alone."""
    true = py(orc, "d1zero")
    assert same(py(orc, "d1zero", "smp_d1_test"), true) == (False, False)
    v, d = py(orc, "d1zero", "cov_no_d1_test")
    assert v.tobytes() == true[0].tobytes() and d["coverage"][0, 1] > true[1]["coverage"][0, 1]


def test_default_rules_change_nothing(orc):
    for name in ("cov_101", "corridor"):
        assert same(color_ref_py.color_transfer(cases.rig(name), orc, rules=()), color_ref_py.color_transfer(cases.rig(name), orc)) == (True, True)
    with pytest.raises(AssertionError):
        color_ref_py.color_transfer(cases.rig("cov_101"), orc, rules=["no_such_rule"])


# ---- agreement -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cases.NAMES)
def test_the_two_restatements_agree(orc, name):
    assert same(ref(orc, name), py(orc, name)) == (True, True)


# ---- the reference's own code ----------------------------------------------------------------------------------------------------

def test_fixture_covers_every_rig_outside_defined():
    z = np.load(GOLDEN)
    assert tuple(str(n) for n in z["names"]) == tuple(n for n in cases.NAMES if n not in cases.DEFINED)
    assert cases.DEFINED == {f"ns_{k}" for k in cases.NS} and set(cases.FULL) <= set(cases.NAMES) - cases.DEFINED
    assert os.path.getsize(GOLDEN) < 450_000


@pytest.mark.parametrize("name", [n for n in cases.NAMES if n not in cases.DEFINED])
def test_color_ref_equals_reference_fixture(orc, name):
    z = np.load(GOLDEN)
    assert str(z[name + "/inputs"]) == export_cases.sha(export_cases.rig_inputs(cases.rig(name))), "the rig is no longer the one the fixture was made from"
    v, d = ref(orc, name)
    assert cases.equals_fixture(z, name, v)
    plain = np.concatenate([s.verts for s in sensors(orc, name)])
    changed = (v.view(np.uint8).reshape(-1, 16)[:, :3] != plain.view(np.uint8).reshape(-1, 16)[:, :3]).any(axis=1).sum()
    assert int(z[name + "/changed"]) == changed and (changed > 0) == bool(d["pairs"])


def test_generator_reproduces_the_fixture(tmp_path):
    """Reruns the reference on every rig where a checkout is present (the only test here that reads it): byte-identical arrays."""
    if not os.path.exists(os.path.join(REFERENCE, "src", "NativeUtils", "depthprocessing.cpp")):
        pytest.skip("no LiveScan3D checkout at $LIVESCAN3D_REFERENCE; the committed fixture stands for it")
    gen = os.path.join(export_cases.GOLDEN, "make_color_boundary_golden.py")
    subprocess.check_call([sys.executable, gen, REFERENCE, str(tmp_path)], stdout=subprocess.DEVNULL, timeout=600)
    fresh, z = np.load(tmp_path / "color_boundary_ref.npz"), np.load(GOLDEN)
    assert sorted(fresh.files) == sorted(z.files)
    for k in z.files:
        assert fresh[k].dtype == z[k].dtype and fresh[k].tobytes() == z[k].tobytes(), k
