"""The flying-pixel filter's restatement (tests/flying_ref.py) held to the reference's own three-argument filterFlyingPixels
(tests/golden/flying_pixels_ref.npz and flying_pixels_digests.json, made by tests/golden/make_flying_golden.py), bit for bit: sizes from
1 x 1 up, r in {1, 2, 3, 7} with 2r + 1 equal to, one below and one above a frame side, thr in {-1, 0, 1, 20, 65534, 65535, 70000},
patterns on the strict comparisons, decisions on the unmodified map, scene / noise / ring frames, an all-zero frame; the third argument
ignored.  Also host state that needs no device: $LSN_FLYING_PIXELS parsing, the lsnSetFlyingPixelFilter round trip, the new exports with
NULL / zero arguments and without a GPU."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import flying_cases, flying_ref as ref
from tests.support import ROOT, child

GOLDEN = os.path.join(ROOT, "tests", "golden", "flying_pixels_ref.npz")
DIGESTS = os.path.join(ROOT, "tests", "golden", "flying_pixels_digests.json")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _cases(g):
    names = [str(x) for x in g["frame_names"]]
    for c in range(len(g["case_r"])):
        name = names[int(g["case_frame"][c])]
        yield c, name, g[f"frame_{name}"], int(g["case_r"][c]), int(g["case_thr"][c]), g[f"result_{c}"]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<u2").tobytes()).hexdigest()


def test_fixture_is_what_the_generator_describes(golden):
    frames = flying_cases.small_frames()
    assert [str(x) for x in golden["frame_names"]] == list(frames)
    for name, d in frames.items():
        assert golden[f"frame_{name}"].tobytes() == d.tobytes() and golden[f"frame_{name}"].shape == d.shape, name
    assert [(n, r, t) for _, n, _, r, t, _ in _cases(golden)] == flying_cases.small_cases(frames)
    assert golden["third_arguments"].tolist() == [0, 4, 1000] and bool(golden["third_argument_ignored"].all())
    assert os.path.getsize(GOLDEN) < 500 * 1024


def test_fixture_covers_the_cases(golden):
    sizes = {golden[f"frame_{n}"].shape[::-1] for n in (str(x) for x in golden["frame_names"])}
    assert {(1, 1), (2, 2), (3, 3), (3, 7), (17, 5), (37, 29), (513, 9), (96, 80)} <= sizes
    seen, rs, thrs = set(), set(), set()
    for c, name, d, r, thr, res in _cases(golden):
        h, w = d.shape
        rs.add(r)
        thrs.add(thr)
        for side in (w, h):
            seen.add({0: "equal", 1: "below", -1: "above"}.get(side - (2 * r + 1), "other"))
        changed = int((res != d).sum())
        if 0 < changed < d.size // 2:
            seen.add("some_removed")
        if name.startswith("all_zero"):
            assert not res.any()
        if 2 * r + 1 > w or 2 * r + 1 > h:
            assert res.tobytes() == d.tobytes(), (name, r)       # a frame smaller than the window is left as it is
        assert res[:r].tobytes() == d[:r].tobytes() and res[h - r:].tobytes() == d[h - r:].tobytes()             # the border band
        assert res[:, :r].tobytes() == d[:, :r].tobytes() and res[:, max(w - r, 0):].tobytes() == d[:, max(w - r, 0):].tobytes()
    assert rs == {1, 2, 3, 7} and thrs == {-1, 0, 1, 20, 65534, 65535, 70000}
    assert {"equal", "below", "above", "some_removed"} <= seen


def test_patterns_land_on_the_strict_comparisons(golden):
    """What the reference itself did with the patterns (the fixture's results, not the restatement's)."""
    names = [str(x) for x in golden["frame_names"]]
    res = {(n, r, t): x for _, n, _, r, t, x in _cases(golden)}
    d = golden["frame_step_edge_17x5"]
    assert res[("step_edge_17x5", 1, 20)].tobytes() == d.tobytes()                           # 3 of 8 differ: kept
    corner = res[("step_corner_17x5", 1, 20)]
    assert corner[2, 8] == 0 and int((corner != golden["frame_step_corner_17x5"]).sum()) == 1    # 5 of 8: removed, and only it
    assert res[("checkerboard_37x29", 1, 20)].tobytes() == golden["frame_checkerboard_37x29"].tobytes()   # 4 of 8: kept
    ex, exr = golden["frame_exact_thresholds_37x29"], res[("exact_thresholds_37x29", 1, 20)]
    assert exr[3, 3] == 1020 and exr[3, 7] == 0 and exr[3, 19] == 980 and exr[3, 23] == 0   # |difference| == thr kept, thr + 1 removed
    z = res[("zero_against_65535_37x29", 1, 65534)]
    assert z[4, 4] == 0 and res[("zero_against_65535_37x29", 1, 65535)][4, 4] == 65535
    assert res[("zero_against_65535_37x29", 1, 65535)].tobytes() == golden["frame_zero_against_65535_37x29"].tobytes()
    lines = res[("lines_and_dots_37x29", 1, 20)]
    assert lines[5, 20] == 0 and lines[10, 9] == 0 and lines[10, 8] == 1000 == lines[10, 10]   # an isolated pixel and a one-pixel line (6 of 8) go, the pixels beside the line (3 of 8) stay
    for name in ("two_levels_37x29", "two_levels_holes_37x29"):                               # decisions on the unmodified map
        assert ref.filter_in_place_sequential(golden[f"frame_{name}"], 1, 20).tobytes() != res[(name, 1, 20)].tobytes()
    # thr = -1: every examined pixel differs from every neighbour; thr = 70000: none does
    d = golden["frame_scene_96x80"]
    assert not res[("scene_96x80", 1, -1)][1:-1, 1:-1].any() and res[("scene_96x80", 1, 70000)].tobytes() == d.tobytes()
    assert len(names) >= 25


def test_restatement_equals_the_reference(golden):
    n = 0
    for c, name, d, r, thr, res in _cases(golden):
        assert ref.filter(d, r, thr).tobytes() == res.tobytes(), (c, name, r, thr)
        assert ref.removed_count(d, r, thr) == int(((d != 0) & (res == 0)).sum())
        n += 1
    assert n >= 600


def test_restatement_equals_the_reference_on_the_digest_frames():
    doc = json.load(open(DIGESTS))
    assert doc["third_arguments"] == [0, 4, 1000]
    want = flying_cases.digest_cases()
    assert [(e["frame"], e["r"], e["thr"]) for e in doc["cases"]] == want
    frames = {}
    sizes = set()
    for e in doc["cases"]:
        key = json.dumps(e["frame"], sort_keys=True)
        if key not in frames:
            frames[key] = flying_cases.digest_frame(e["frame"])
        d = frames[key]
        sizes.add((e["frame"]["w"], e["frame"]["h"]))
        assert e["third_argument_ignored"] is True
        assert _sha(d) == e["input_sha256"] and e["valid"] == int((d != 0).sum())
        got = ref.filter(d, e["r"], e["thr"])
        assert _sha(got) == e["result_sha256"], (e["frame"], e["r"], e["thr"])
        assert ref.removed_count(d, e["r"], e["thr"]) == e["removed"]
    assert sizes == set(flying_cases.DIGEST_SIZES)
    # the seed-1 ring at the client's defaults: every sensor loses 8.9 - 15.0 % of its valid pixels; a noise frame nearly everything
    ring = [e for e in doc["cases"] if e["frame"]["kind"] == "scene" and e["frame"]["w"] == 512 and (e["r"], e["thr"]) == (1, 20)]
    assert len(ring) == 8 and all(0.089 <= e["removed"] / e["valid"] <= 0.151 for e in ring)
    assert (ring[0]["valid"], ring[0]["removed"]) == (111905, 11983)
    noise = [e for e in doc["cases"] if e["frame"]["kind"] == "noise" and e["frame"]["w"] == 512 and (e["r"], e["thr"]) == (1, 20)]
    assert noise and noise[0]["removed"] / noise[0]["valid"] > 0.98


def test_not_idempotent_and_off():
    d = flying_cases.digest_frame(dict(kind="scene", seed=1, tick=0, sensor=0, of=8, w=512, h=424))
    once = ref.filter(d, 1, 20)
    assert ref.removed_count(once, 1, 20) == 889            # a second pass removes more: a tick must apply the filter exactly once
    for r in (0, -1, -7):
        assert ref.filter(d, r, 20).tobytes() == d.tobytes()
    packed, removed = ref.filter_packed(np.concatenate([d.ravel(), d[:100].ravel()]).view(np.uint8), [512, 512], [424, 100], 1, 20)
    assert removed[0] == 11983 and packed.view("<u2")[:d.size].tobytes() == once.tobytes()


# ---- host state of the library: no device needed --------------------------------------------------------------------------------------

DROP = ("LSN_FLYING_PIXELS",)   # the children start without the switch of this shell


def test_environment_switch_parsing():
    # the child reads the switch by setting it and setting it back: nothing else runs in that process
    code = "from livescan3d_amd import native; p = native.set_flying_pixel_filter(0, 0); native.set_flying_pixel_filter(*p); print(p)"
    assert child(code, {}, drop=DROP)[0] == "(0, 0)"
    assert child(code, {"LSN_FLYING_PIXELS": "1,20"}, drop=DROP)[0] == "(1, 20)"
    assert child(code, {"LSN_FLYING_PIXELS": " 3 , -1 "}, drop=DROP)[0] == "(3, -1)"
    for bad in ("one", "1", "1,20x", "1;20", "1,2.5", ","):
        out, err = child(code, {"LSN_FLYING_PIXELS": bad}, drop=DROP)
        assert out == "(0, 0)" and "LSN_FLYING_PIXELS" in err, bad
    assert child(code, {"LSN_FLYING_PIXELS": ""}, drop=DROP)[0] == "(0, 0)"


def test_switch_round_trip():
    from livescan3d_amd import native
    L = native.lib()
    first = native.set_flying_pixel_filter(2, 35)
    try:
        assert native.set_flying_pixel_filter(-4, 70000) == (2, 35)
        assert L.lsnSetFlyingPixelFilter(1, 20, None, None) == 0            # either output may be NULL
        n, t = C.c_int(-9), C.c_int(-9)
        assert L.lsnSetFlyingPixelFilter(7, 0, C.byref(n), None) == 0 and n.value == 1
        assert L.lsnSetFlyingPixelFilter(0, 0, None, C.byref(t)) == 0 and t.value == 0
    finally:
        native.set_flying_pixel_filter(*first)
    assert native.set_flying_pixel_filter(*first) == first


def test_new_exports_survive_null_and_zero_arguments():
    from livescan3d_amd import native
    L = native.lib()
    for sym in ("lsnFusionFlyingPixels", "lsnFusionFlyingDiagnostics", "lsnSetFlyingPixelFilter", "lsnTickSetFlyingPixels"):
        assert sym in native.EXPORTS and hasattr(L, sym)
    assert L.lsnFusionFlyingPixels(None, 1, 20, None, None, None) == -1 and "null argument" in native.last_error()
    assert L.lsnFusionFlyingPixels(None, 0, 0, None, None, None) == -1
    out = (C.c_int * 4)()
    assert L.lsnFusionFlyingDiagnostics(None, 0, out, None) == -1 and "lsnFusionFlyingDiagnostics" in native.last_error()
    assert L.lsnFusionFlyingDiagnostics(None, -1, None, None) == -1
    assert L.lsnTickSetFlyingPixels(None, 1, 20) == -1 and "lsnTickSetFlyingPixels" in native.last_error()
    assert L.lsnTickSetFlyingPixels(None, 0, 0) == -1


def _no_gpu():
    from livescan3d_amd import native
    return native.device_count() <= 0


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a machine without a GPU (tests/test_flying_gpu.py covers the calls where there is one)")
def test_filtered_exports_fail_loudly_without_a_gpu():
    """Like the other exports: no CPU path."""
    from livescan3d_amd import native, synth
    rig = synth.make_rig("scene", 2, 32, 24)
    with pytest.raises(native.NativeUtilsError):
        native.radial_correction(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, flying_pixels=(1, 20))
    with pytest.raises(native.NativeUtilsError):
        native.correct_and_generate_mesh(rig.depth_maps, rig.depth_colors, rig.widths, rig.heights, rig.intr, rig.wt, rig.bounds, flying_pixels=(1, 20))
    with pytest.raises(native.NativeUtilsError):
        native.FusionPlan(0, 1, [32], [24])
    assert native.set_flying_pixel_filter(0, 0) == (0, 0)                   # the switch was restored on the way out
