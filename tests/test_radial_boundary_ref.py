"""The boundary cases of radial correction on the CPU (no GPU): every case of tests/radial_cases.py is held to what it is named for -- a
witness computed from the float32 warp target or from the numpy model of the closing rounds -- and the oracle is held to the reference's
own depthMapAndColorSetRadialCorrection (tests/golden/radial_boundary_ref.npz) on all of them.  A case whose input is weakened fails its
witness here, not a comparison on the GPU.

What is compared with what:
  * np_warp_target (vectorised) with py_radial's loop, one valid pixel at a time, on 17 x 13 frames under ordinary, folding, overflowing
    and NaN calibrations;
  * np_radial (np_warp + round_model: the rounds' fixed point) with the oracle on every case -- the design's claim that the rounds
    reach the sequential loop's state -- and with py_radial on the cases small enough for its Python loop;
  * the oracle with py_radial on those small cases, and with the fixture on every case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import export_cases, radial_cases as rc
from tests.depth_ref import np_warp_target, py_radial

GOLDEN = os.path.join(export_cases.GOLDEN, "radial_boundary_ref.npz")
REFERENCE = os.environ.get("LIVESCAN3D_REFERENCE", "/root/reference")
_Z = np.load(GOLDEN)
# py_radial walks every pixel in Python (about 10 us each): the cases of at most this many pixels run through it, which leaves out
# code16 (786 k), the capacity, frames and chunks cases and the larger align / rounds rigs -- np_radial and the oracle cover those
PY_LOOP_PIXELS = 13000
SMALL = ["src4_lo", "src4_hi", "src5_lo", "src5_hi", "src4_lo_rig", "src4_hi_rig", *[f"ends_{w}x{h}" for w, h in rc.ENDS_SIZES],
         "rounds_64x48", "rounds_61x37", "calib_identity", "calib_kinect", "calib_src4", "calib_src5"]      # (named: no case is built at import)


@functools.lru_cache(maxsize=None)
def oracle_out(name):
    """The oracle's (depth u16, colours u8) of a case, tick after tick."""
    from oracle import orc
    orc.build()
    res = [orc.radial_correction(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr) for r in rc.ticks(name)]
    return np.concatenate([d for d, _ in res]).view("<u2"), np.concatenate([c for _, c in res])


def _per_frame(name, fn):
    dd, cc = [], []
    for rig in rc.ticks(name):
        for d, c, i in rc.frames_of(rig):
            a, b = fn(d, c, i)
            dd.append(np.asarray(a).ravel())
            cc.append(np.asarray(b).ravel())
    return np.concatenate(dd), np.concatenate(cc)


def equals_fixture(name, depth, colors):
    return rc.equals_fixture(_Z, name, depth, colors)


# ---- the fixture and the oracle ------------------------------------------------------------------------------------------------------

def test_fixture_holds_every_case_and_each_case_has_one_calibration():
    assert tuple(str(n) for n in _Z["names"]) == rc.NAMES
    assert {rc.FAMILY[n] for n in rc.NAMES} == {"sources", "code16", "ends", "align", "rounds", "capacity", "frames", "chunks", "calib"}
    for n in rc.NAMES:
        t = rc.ticks(n)
        assert all(np.array_equal(r.intr, t[0].intr) and np.array_equal(r.widths, t[0].widths) and np.array_equal(r.heights, t[0].heights)
                   for r in t), n
        assert export_cases.sha(rc.case_inputs(n)) == str(_Z[n + "/inputs"]), f"{n}: the builder no longer rebuilds the fixture's inputs"
    assert os.path.getsize(GOLDEN) < 256 * 1024


@pytest.mark.parametrize("name", rc.NAMES)
def test_oracle_equals_reference_fixture(orc, name):
    assert equals_fixture(name, *oracle_out(name))


@pytest.mark.parametrize("name", rc.NAMES)
def test_rounds_reach_the_sequential_fixed_point(orc, name):
    """np_radial = the float32 warp target + the model of the rounds, against the oracle's sequential loop."""
    d, c = _per_frame(name, rc.np_radial)
    want_d, want_c = oracle_out(name)
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_and_model_equal_py_radial_on_the_small_cases(orc, name):
    d, c = _per_frame(name, py_radial)
    want_d, want_c = oracle_out(name)
    assert np.array_equal(d, want_d) and np.array_equal(c, want_c)


def test_generator_reproduces_the_fixture(tmp_path):
    if not os.path.exists(os.path.join(REFERENCE, "src", "NativeUtils", "depthprocessing.cpp")):
        pytest.skip("no LiveScan3D checkout at $LIVESCAN3D_REFERENCE; the committed fixture stands for it")
    gen = os.path.join(export_cases.GOLDEN, "make_radial_boundary_golden.py")
    subprocess.check_call([sys.executable, gen, REFERENCE, str(tmp_path)], stdout=subprocess.DEVNULL, timeout=900)
    fresh = np.load(tmp_path / "radial_boundary_ref.npz")
    assert sorted(fresh.files) == sorted(_Z.files)
    for k in _Z.files:
        assert fresh[k].dtype == _Z[k].dtype and fresh[k].tobytes() == _Z[k].tobytes(), k


# ---- the warp target -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", range(8))
def test_warp_target_equals_py_radial_one_pixel_at_a_time(k):
    w, h = 17, 13
    intr = [export_cases._intr(w, h), export_cases._intr(w, h, r2=3.0, r4=0, r6=0), export_cases._intr(w, h, r2=-40.0),
            export_cases._intr(w, h, r2=1e12), export_cases._intr(w, h, r6=-1e30), export_cases._intr(w, h, cx=export_cases.NAN),
            export_cases._intr(w, h, fx=0.0, cx=14.0), np.float32([8, 6, 16, 16, 0.68, 0, 0])][k]
    dst = np_warp_target(w, h, intr)
    rgb = np.zeros((h, w, 3), np.uint8)
    for p in range(w * h):
        d = np.zeros(w * h, np.uint16)
        d[p] = 7
        out = py_radial(d.reshape(h, w), rgb, intr)[0].ravel()
        assert np.flatnonzero(out).tolist() == ([int(dst[p])] if dst[p] >= 0 else []), (k, p)
    count, cand = rc.sources(w, h, intr)
    assert count.sum() == (dst >= 0).sum() and all(sorted(np.flatnonzero(dst == q).tolist(), reverse=True) == cand[q][cand[q] >= 0].tolist()
                                                    for q in range(w * h))


# ---- sources per destination ---------------------------------------------------------------------------------------------------------

def test_bisection_finds_the_two_neighbouring_calibrations():
    lo, hi = rc.bisect_r2()
    assert (lo, hi) == (rc.R2_MAX4, rc.R2_MIN5) and np.nextafter(lo, np.float32(1)) == hi
    assert rc.max_sources(lo) == 4 and rc.max_sources(hi) == 5


@pytest.mark.parametrize("r2,most", [(np.float32(0.21), 4), (rc.R2_MAX4, 4), (rc.R2_MIN5, 5), (np.float32(0.68), 5)])
def test_source_planes_make_every_candidate_win(r2, most):
    count, cand = rc.sources(rc.SRC_W, rc.SRC_H, rc.src_intr(r2))
    assert count.max() == most and all((count == k).sum() >= 1 for k in (2, 3, 4))
    # the source sets of distinct destinations are disjoint: a plane is well defined
    s = cand[cand >= 0]
    assert len(np.unique(s)) == len(s)
    for j, d in enumerate(rc.src_planes(r2)):
        win = rc.winners(d, cand)
        for k in (2, 3, 4, 5)[:most - 1]:
            got = win[count == k]
            assert (got == (j if j < k else -1)).all() and len(got) >= 1, (r2, j, k)
        # ... and the colour names the winner: no two sources of one destination share a colour
        col = rc.colour_of(rc.SRC_W * rc.SRC_H)
        for q in np.flatnonzero(count >= 2):
            assert len({tuple(col[s]) for s in cand[q][:count[q]]}) == count[q]


def test_source_cases_are_those_planes():
    for name, r2 in (("src4_lo", 0.21), ("src4_hi", rc.R2_MAX4), ("src5_lo", rc.R2_MIN5), ("src5_hi", 0.68)):
        planes = rc.src_planes(np.float32(r2))
        assert [f[0][0].tolist() for f in map(rc.frames_of, rc.ticks(name))] == [p.tolist() for p in planes]
    for name, r2 in (("src4_lo_rig", 0.21), ("src4_hi_rig", rc.R2_MAX4)):
        (rig,) = rc.ticks(name)
        assert [d.tolist() for d, _, _ in rc.frames_of(rig)] == [p.tolist() for p in rc.src_planes(np.float32(r2))]


# ---- the 16-bit code's edge ------------------------------------------------------------------------------------------------------------

def test_code16_reaches_both_sides_of_the_codes_edge_without_overflow():
    seen = set()
    t0, t1 = rc.ticks("code16")
    for s, (cx, cy) in enumerate(rc.C16_CALIB):
        count, cand = rc.sources(rc.C16_W, rc.C16_H, rc.c16_intr(cx, cy))
        assert count.max() <= 4
        rel = rc.rel_of(cand)[:, :2][cand[:, :2] >= 0]
        seen |= set(np.unique(rel).tolist())
        # plane 1: where there is a second candidate it wins, a far one included
        d1 = rc.frames_of(t1)[s][0]
        win = rc.winners(d1, cand)
        assert (win[count >= 2] == 1).all() and (win[count == 1] == -1).all()
        assert (rc.winners(rc.frames_of(t0)[s][0], cand)[count >= 1] == 0).all()
    assert set(rc.C16_RELS) <= seen, sorted(set(rc.C16_RELS) - seen)
    # each of the eight values as a FIRST and as a SECOND candidate somewhere in the rig
    firsts, seconds = set(), set()
    for cx, cy in rc.C16_CALIB:
        count, cand = rc.sources(rc.C16_W, rc.C16_H, rc.c16_intr(cx, cy))
        rel = rc.rel_of(cand)
        firsts |= set(np.unique(rel[:, 0][cand[:, 0] >= 0]).tolist())
        if cand.shape[1] > 1:
            seconds |= set(np.unique(rel[:, 1][cand[:, 1] >= 0]).tolist())
    assert set(rc.C16_RELS) <= firsts and {32767, 32768, -32767, -32768} <= seconds


# ---- the colour read at the ends of a frame ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", rc.ENDS_SIZES)
def test_ends_cases_put_the_first_and_the_last_pixel_into_the_output(w, h):
    (rig,) = rc.ticks(f"ends_{w}x{h}")
    frames = rc.frames_of(rig)
    assert [f[0].shape for f in frames] == [(hh, ww) for ww, hh in rc.ends_sizes(w, h)] and frames[2][0].shape == (1, 1)
    offs = np.concatenate([[0], np.cumsum(rig.widths.astype(np.int64) * rig.heights)])
    assert offs[3] % 16 == 1 and (3 * offs[3]) % 16 == 3, "behind the 1 x 1 frame: an odd pixel offset, colour at 3 modulo 16"
    for k in rc.ENDS_PLACES:
        d, c, intr = frames[k]
        count, cand = rc.sources(w, h, intr)
        assert cand[0, 0] == 0 and cand[-1, 0] == w * h - 1 and d.flat[0] != 0 and d.flat[-1] != 0
        assert c.reshape(-1, 3)[-1].any() and c.reshape(-1, 3)[0].any(), "a colour of zero would hide a read that came back empty"


def test_small_list_is_the_cases_below_the_python_loops_limit():
    assert SMALL == [n for n in rc.NAMES if rc.pixels(n) <= PY_LOOP_PIXELS]


# ---- pointer alignment ---------------------------------------------------------------------------------------------------------------

def test_align_cases_are_a_vec_capable_and_a_ragged_rig_and_the_offsets_cover_both_sides():
    vec, ragged = rc.ticks("align_vec"), rc.ticks("align_ragged")
    assert len(vec) == len(ragged) == 2
    assert all(w % 8 == 0 for w in vec[0].widths.tolist()) and rc.pixels("align_vec") // 2 % 8 == 0, "vec-capable: every width and the tick"
    assert ragged[0].widths.tolist() == [61, 64, 250] and any(w % 8 for w in ragged[0].widths.tolist())
    assert all(r.heights.tolist() == [48] * 3 for r in vec + ragged)
    ok = [o for o in rc.ALIGN_OFFSETS if rc.vec_eligible(o)]
    assert ok == [(0, 0), (0, 8)] and len(rc.ALIGN_OFFSETS) == 56, "two pairs take the wide kernels, 54 must take the narrow ones"
    # every depth offset that is even and below 16, every colour residue class modulo 8 that is not 0 at least once
    assert set(rc.ALIGN_DEPTH_OFFSETS) == set(range(0, 16, 2)) and {c % 8 for c in rc.ALIGN_COLOUR_OFFSETS} >= {0, 1, 3, 5, 7}
    # out of place the output's offsets are OFFSETS[(5 i + 3) % 56]: all four combinations of eligible / not, input against output
    pairs = {(rc.vec_eligible(o), rc.vec_eligible(rc.ALIGN_OFFSETS[(5 * i + 3) % 56])) for i, o in enumerate(rc.ALIGN_OFFSETS)}
    assert pairs >= {(True, False), (False, True), (False, False)}
    for rig in vec + ragged:
        for d, _, _ in rc.frames_of(rig):
            assert 0.1 < (d == 0).mean() < 0.3, "holes for the closing on every frame"


# ---- boundary values in the rounds -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", rc.ROUNDS_SIZES)
def test_rounds_cases_feed_filled_boundary_values_to_the_next_evaluation(orc, w, h):
    (rig,) = rc.ticks(f"rounds_{w}x{h}")
    od = oracle_out(f"rounds_{w}x{h}")[0].reshape(4, h, w)
    edges = rc.band_edge_rows(h)
    assert {y % 6 for y in edges} >= {0, 5} and 1 in edges and h - 2 in edges
    for s, (d, c, intr) in enumerate(rc.frames_of(rig)):
        U, UC = rc.np_warp(d, c, intr)
        assert np.array_equal(U, d), "the identity moves nothing"
        D, C, sizes = rc.round_model(U, UC)
        assert np.array_equal(D, od[s])
        if s < 3:
            assert set(np.unique(d).tolist()) <= set(rc.VALUE_SETS[s].tolist()) | {0}
            with_pred, order_decides, window_decides = rc.order_witness(U, UC, od[s])
            assert all(with_pred[y] > 0 and order_decides[y] > 0 for y in edges), (s, [(y, with_pred[y], order_decides[y]) for y in edges])
            # the window test on a FILLED value decides (a filled predecessor rejected, or an original neighbour's verdict turned): on
            # every band-edge row of the wide frames; the narrow frame has 98 such rows of 12 holes in three runs of four, there on
            # at least a third of the rows of either residue and on row 1
            if w >= 48:
                assert all(window_decides[y] > 0 for y in edges), (s, [y for y in edges if not window_decides[y]])
            else:
                for res in (0, 5):
                    rows = [y for y in edges if y % 6 == res]
                    assert 3 * sum(window_decides[y] > 0 for y in rows) >= len(rows), (s, res)
                assert window_decides[1] > 0, s
            assert len(sizes) > 3, "longer than the two grid-wide rounds"
        else:
            # the chain: one fill per round
            assert len(sizes) >= h - 4 and len(sizes) > (256 if h == 300 else 64), len(sizes)
    assert set(np.unique(rc.frames_of(rig)[0][1]).tolist()) == {0, 1, 254, 255}


# ---- list capacities -------------------------------------------------------------------------------------------------------------------

def test_capacity_cases_lie_on_either_side_of_the_round_lists_capacity(orc):
    """The model's round lists (entries = distinct pixels here: a hole row's fill lists its right neighbour alone), 189 rounds each:
    cap_over 15120 entries in the first list, 15040, 14960 ... in the next (80 fewer per round), at least 1.5 x 8192 = 12288 for 36 rounds;
    cap_under 5103 in the first, 5076, 5049 ... (27 fewer per round), below 8192 / 1.5 = 5461 throughout."""
    over = rc.round_model(*rc.np_warp(*rc.frames_of(rc.ticks("cap_over")[0])[0]))[2]
    under = rc.round_model(*rc.np_warp(*rc.frames_of(rc.ticks("cap_under")[0])[0]))[2]
    print("cap_over", over[:8], len(over), "cap_under", under[:8], len(under))
    assert all(e >= 1.5 * rc.FIX_LIST for e, _ in over[2:8]), over[:8]
    assert all(e <= rc.FIX_LIST / 1.5 for e, _ in under) and len(under) > 100 and under[5][0] > 4000, under[:8]


# ---- 128 / 129 frames, the chunked band list, calibration changes --------------------------------------------------------------------

def test_frames_cases_are_128_and_129_frames():
    assert len(rc.ticks("frames128")) * rc.ticks("frames128")[0].n == 128 and len(rc.ticks("frames129")) * rc.ticks("frames129")[0].n == 129
    for n in ("frames128", "frames129"):
        assert all(r.widths.tolist() == [32] * r.n and r.heights.tolist() == [27] * r.n for r in rc.ticks(n))
        d = oracle_out(n)[0]
        assert (d != np.concatenate([r.depth_maps.view("<u2") for r in rc.ticks(n)])).mean() > 0.05, "the correction moves and closes pixels"


def test_chunks_case_outgrows_one_pass_of_the_band_list():
    (rig,) = rc.ticks("chunks")
    d = rc.frames_of(rig)[0][0]
    valid = (d != 0).astype(np.int64)
    nv = sum(np.roll(np.roll(valid, -dy, axis=0), -dx, axis=1) for dx, dy in rc.SHIFTS)
    cand = (d == 0)[1:-1, 1:-1] & (nv[1:-1, 1:-1] >= 5)
    assert cand[1::2].all() and not cand[0::2].any(), "every interior pixel of alternate rows (y = 2, 4 .. 24)"
    # twelve-row bands start at y = 0, 12, 24 and list rows y0 .. y0 + 7, then y0 + 8 .. y0 + 11: the second chunk's first row is a hole row
    assert 8192 // rc.CHUNK_W == 8 and all((d[y0 + 8, 1:-1] == 0).all() for y0 in (0, 12))
    assert 12 * rc.CHUNK_W > 8192 >= 6 * rc.CHUNK_W, "twelve rows are listed in chunks of eight, the default six in one pass"


def test_calibration_sequence_crosses_the_overflow_flag_both_ways():
    most = [int(rc.sources(rc.SRC_W, rc.SRC_H, rc.calib_intr(k))[0].max()) for k in rc.CALIB_SEQUENCE]
    assert most[0] == 1 and most[2:5] == [4, 5, 4] and most[1] <= 4 and most[5] == most[1]
    assert [(a > 4) != (b > 4) for a, b in zip(most, most[1:])] == [False, False, True, True, False]
