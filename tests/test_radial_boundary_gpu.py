"""Radial correction (csrc/radial.hip) on the boundary cases of tests/radial_cases.py, bit for bit against what the reference's own
depthMapAndColorSetRadialCorrection returned (tests/golden/radial_boundary_ref.npz; the oracle's output is first held to the fixture and
then compared, so that a failure names pixels).  Every case runs through the host export, FusionPlan.radial_correct (in place) and
radial_correct_to (out of place, between guard bands) under every closing and warp switch; the families whose decision lies in how a
batch is handed over -- pointer offsets, batch sizes around 128 frames, round lists at their real capacity, a calibration that changes
on a live plan -- have tests of their own.  tests/test_radial_boundary_ref.py proves on the CPU that each case reaches what it is named
for.  Nothing here has a tolerance."""
import functools
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import radial_cases as rc
from tests.support import GUARD, PATTERN

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radial_boundary_ref.npz")
SWITCHES = {"two-pass": {}, "tiny-lists": {"LSN_RADIAL_TINY_LISTS": "1"}, "wavefront": {"LSN_RADIAL_CLOSE": "wavefront"},
            "four-row-bands": {"LSN_RADIAL_BAND_ROWS": "4"}, "atomic-warp": {"LSN_RADIAL_FORCE_ATOMIC": "1"}}

_want = {}


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(GOLDEN)


def want(orc, name):
    """Per tick (depth bytes u8, colours u8) of a case: the oracle's, held to the reference's fixture.  Computed once, never changed."""
    if name not in _want:
        res = [orc.radial_correction(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr) for r in rc.ticks(name)]
        assert rc.equals_fixture(_fixture(), name, np.concatenate([d for d, _ in res]), np.concatenate([c for _, c in res])), \
            f"{name}: the oracle and the reference's fixture disagree"
        for d, c in res:
            d.setflags(write=False)
            c.setflags(write=False)
        _want[name] = res
    return _want[name]


def same(got_d, got_c, want_dc, what):
    got_d, got_c = np.asarray(got_d).view(np.uint8).ravel(), np.asarray(got_c).ravel()
    wd, wc = np.asarray(want_dc[0]).view(np.uint8).ravel(), np.asarray(want_dc[1]).ravel()
    bad = np.flatnonzero(got_d.view("<u2") != wd.view("<u2"))
    assert not len(bad), f"{what}: {len(bad)} depths differ, first at pixels {bad[:6].tolist()}: {got_d.view('<u2')[bad[:6]].tolist()} for {wd.view('<u2')[bad[:6]].tolist()}"
    bad = np.flatnonzero((got_c != wc).reshape(-1, 3).any(axis=1))
    assert not len(bad), f"{what}: {len(bad)} colours differ, first at pixels {bad[:6].tolist()}: {got_c.reshape(-1, 3)[bad[:6]].tolist()} for {wc.reshape(-1, 3)[bad[:6]].tolist()}"


class Batch:
    """A plan for T ticks of a rig's sizes.  place() copies the ticks into fresh pattern-filled buffers at a byte offset behind a guard
    band; correct() runs in place or out of place on such buffers and holds the bytes around the output ranges to the pattern."""

    def __init__(self, torch, rig, n_ticks):
        self.torch, self.T = torch, n_ticks
        self.plan = native.FusionPlan(0, n_ticks, rig.widths, rig.heights)
        self.npix = self.plan.pixels_per_tick
        self.stream = int(torch.cuda.current_stream().cuda_stream)

    def upload(self, ticks):
        from livescan3d_amd.fusion import upload_rigs
        d, c = upload_rigs(ticks, self.T)
        return d.view(self.torch.uint8).ravel(), c.ravel()

    def place(self, flat, off):
        buf = self.torch.full((GUARD + off + flat.numel() + GUARD,), PATTERN, dtype=self.torch.uint8, device="cuda")
        buf[GUARD + off:GUARD + off + flat.numel()] = flat
        return buf

    def blank(self, nbytes, off):
        return self.torch.full((GUARD + off + nbytes + GUARD,), PATTERN, dtype=self.torch.uint8, device="cuda")

    @staticmethod
    def _intact(buf, off, nbytes):
        return bool((buf[:GUARD + off] == PATTERN).all().item()) and bool((buf[GUARD + off + nbytes:] == PATTERN).all().item())

    def correct(self, intr, dev_d, dev_c, in_off=(0, 0), out_off=None, two_pass=True):
        """dev_d / dev_c: the ticks' bytes on the device.  out_off None: in place at byte offsets in_off = (depth, colour); else out of
        place from in_off to out_off.  Returns (depth bytes [T, 2 npix], colours [T, 3 npix]) as numpy."""
        nd, nc = dev_d.numel(), dev_c.numel()
        bd, bc = self.place(dev_d, in_off[0]), self.place(dev_c, in_off[1])
        pd, pc = bd.data_ptr() + GUARD + in_off[0], bc.data_ptr() + GUARD + in_off[1]
        if out_off is None:
            self.plan.radial_correct(intr, pd, pc, self.stream)
            od, oc, oo = bd, bc, in_off
        else:
            od, oc, oo = self.blank(nd, out_off[0]), self.blank(nc, out_off[1]), out_off
            self.plan.radial_correct_to(intr, pd, pc, od.data_ptr() + GUARD + oo[0], oc.data_ptr() + GUARD + oo[1], self.stream)
        self.torch.cuda.synchronize()
        assert self._intact(od, oo[0], nd) and self._intact(oc, oo[1], nc), f"bytes around the output changed (offsets {in_off} -> {out_off})"
        if out_off is not None:
            assert self._intact(bd, in_off[0], nd) and self._intact(bc, in_off[1], nc)
            assert self.torch.equal(bd[GUARD + in_off[0]:GUARD + in_off[0] + nd], dev_d) and self.torch.equal(bc[GUARD + in_off[1]:GUARD + in_off[1] + nc], dev_c), \
                "out of place: the input was touched"
        if two_pass:
            assert self.plan.radial_counters_left(self.stream) == 0, "the closing chain left work counters behind"
        return (od[GUARD + oo[0]:GUARD + oo[0] + nd].cpu().numpy().reshape(self.T, -1), oc[GUARD + oo[1]:GUARD + oo[1] + nc].cpu().numpy().reshape(self.T, -1))

    def close(self):
        self.plan.close()


def run_case(torch, orc, name, two_pass=True, host_ticks=1):
    """Case `name` through the three entry points under the switches that are set."""
    ticks, expect = rc.ticks(name), want(orc, name)
    for k in range(min(host_ticks, len(ticks))):
        r = ticks[k]
        same(*native.radial_correction(r.depth_maps, r.depth_colors, r.widths, r.heights, r.intr), expect[k], f"{name}: host export, tick {k}")
    b = Batch(torch, ticks[0], len(ticks))
    try:
        dev = b.upload(ticks)
        for out_off, what in ((None, "in place"), ((0, 0), "out of place")):
            got_d, got_c = b.correct(ticks[0].intr, *dev, out_off=out_off, two_pass=two_pass)
            for k in range(len(ticks)):
                same(got_d[k], got_c[k], expect[k], f"{name}: {what}, tick {k}")
    finally:
        b.close()


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", rc.NAMES)
def test_every_case_on_every_entry_point_and_switch(gpu, orc, monkeypatch, name, switch):
    import torch
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    run_case(torch, orc, name, two_pass=switch != "wavefront", host_ticks=len(rc.ticks(name)) if switch == "two-pass" and len(rc.ticks(name)) <= 5 else 1)


@pytest.mark.parametrize("name,rows", [("chunks", "12"), ("rounds_64x48", "1"), ("rounds_61x37", "1"), ("rounds_24x300", "12"), ("code16", "12")])
def test_band_heights_that_chunk_the_candidate_list_and_single_row_bands(gpu, orc, monkeypatch, name, rows):
    """Twelve rows of the 1024-wide frame are more pixels than the band's candidate list holds (8192): the rows are listed eight at a
    time.  One-row bands: every hole row is a band of its own, all its neighbours are halo."""
    import torch
    monkeypatch.setenv("LSN_RADIAL_BAND_ROWS", rows)
    run_case(torch, orc, name)


OFFSETS = rc.ALIGN_OFFSETS


@pytest.mark.parametrize("name", ["align_vec", "align_ragged"])
def test_every_pointer_offset_in_place_and_out_of_place(gpu, orc, name):
    """A vec-capable rig handed over at pointers that are not 16-byte (depth) / 8-byte (colour) aligned takes the narrow kernels, and
    the lead handling of store_band_run / store_run then writes the first bytes of every row run one by one: 54 of the 56 offset
    pairs.  Every depth offset with every colour offset in place; out of place the input at one pair of offsets and the output at
    another, independently.  Held: the result and the bytes around it.  Not held, because no output shows it: WHICH kernels ran (with
    vec_ptrs disabled gfx950 completes the wide kernels' misaligned accesses with the same bytes; EXPERIMENTS.md)."""
    import torch
    ticks, expect = rc.ticks(name), want(orc, name)
    b = Batch(torch, ticks[0], len(ticks))
    try:
        dev = b.upload(ticks)
        for i, off in enumerate(OFFSETS):
            for out_off in (None, OFFSETS[(5 * i + 3) % len(OFFSETS)]):
                got_d, got_c = b.correct(ticks[0].intr, *dev, in_off=off, out_off=out_off)
                for k in range(len(ticks)):
                    same(got_d[k], got_c[k], expect[k], f"{name}: offsets {off} -> {out_off}, tick {k}")
    finally:
        b.close()


@pytest.mark.parametrize("switch", [s for s in SWITCHES if s != "two-pass"])
def test_pointer_offsets_under_the_switches(gpu, orc, monkeypatch, switch):
    import torch
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    for name in ("align_vec", "align_ragged"):
        ticks, expect = rc.ticks(name), want(orc, name)
        b = Batch(torch, ticks[0], len(ticks))
        try:
            dev = b.upload(ticks)
            for off, out_off in (((2, 1), None), ((8, 3), None), ((0, 13), (14, 8)), ((6, 0), (0, 7)), ((0, 8), (4, 15))):
                got_d, got_c = b.correct(ticks[0].intr, *dev, in_off=off, out_off=out_off, two_pass=switch != "wavefront")
                for k in range(len(ticks)):
                    same(got_d[k], got_c[k], expect[k], f"{name}: {switch}, offsets {off} -> {out_off}, tick {k}")
        finally:
            b.close()


@pytest.mark.parametrize("n_ticks", [3, 129])
@pytest.mark.parametrize("name", ["cap_over", "cap_under"])
def test_round_lists_at_their_real_capacity(gpu, orc, name, n_ticks):
    """The round lists of close_fix_kernel hold 8192 entries.  The model of the rounds (tests/radial_cases.round_model; the counts are
    asserted by tests/test_radial_boundary_ref.py) gives, for one frame:
      cap_over   15120, 15040, 14960, 14880, 14800, 14720 ... entries in the first lists, 80 fewer per round, above 1.5 x 8192 = 12288
                 for 36 rounds, 189 rounds in all: the list overflows whichever round is the first to be kept in LDS, and the frame is swept;
      cap_under  5103, 5076, 5049, 5022, 4995 ... entries, 27 fewer per round, never above 8192 / 1.5 = 5461, 189 rounds: the lists hold.
    Three frames take the two grid-wide rounds in front of the per-frame kernel, 129 the per-frame kernel alone.
    The frames are 192 x 242 (129 of them: 6.0 M pixels, 30 MB of frames): every changed pixel of a hole row lists one successor, so a
    list holds at most one entry per hole, and the 1.5 x margin above 8192 for the first five lists needs more than 12288 + 5 x 80 holes
    in rows that are a third of the frame -- a 128 x 200 frame has 8316."""
    import torch
    (tick,), (expect,) = rc.ticks(name), want(orc, name)
    b = Batch(torch, tick, n_ticks)
    try:
        dev = b.upload([tick])
        for out_off in (None, (0, 0)):
            got_d, got_c = b.correct(tick.intr, *dev, out_off=out_off)
            assert (got_d == got_d[0]).all() and (got_c == got_c[0]).all(), "equal frames of one batch came back different"
            same(got_d[0], got_c[0], expect, f"{name} x {n_ticks}")
    finally:
        b.close()


@pytest.mark.parametrize("out_of_place", [False, True])
def test_calibration_changes_on_a_live_plan(gpu, orc, out_of_place):
    """One plan, one stream: identity, Kinect-like, the 4-source calibration, the 5-source one (the table overflows: atomicMax path), the
    4-source one again (the overflow flag must fall), Kinect-like again.  The warp tables are rebuilt whenever the intrinsics differ from
    the previous call's."""
    import torch
    b = Batch(torch, rc.ticks("calib_identity")[0], 2)
    try:
        for step, which in enumerate(rc.CALIB_SEQUENCE):
            ticks, expect = rc.ticks("calib_" + which), want(orc, "calib_" + which)
            got_d, got_c = b.correct(rc.calib_intr(which), *b.upload(ticks), out_off=(0, 0) if out_of_place else None)
            for k in range(2):
                same(got_d[k], got_c[k], expect[k], f"call {step} ({which}), tick {k}")
    finally:
        b.close()
