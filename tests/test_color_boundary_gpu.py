"""lsnFusionColorTransfer (csrc/color.hip, csrc/cloud_index.hip) and the host export with bcolor_transfer on the boundary rigs of
tests/color_boundary_cases.py, against the CPU reference (tests/color_ref.py) and, with nothing in between, against what the reference's
own generateMeshFromDepthMaps returned (tests/golden/color_boundary_ref.npz).  Bit for bit: the vertex bytes, the confidence maps, the
coverage table, the pairs in the order they were chosen, the transforms.  Nothing here has a tolerance.
tests/test_color_boundary_ref.py holds the rigs to what they claim to reach and to decide: both sides of the three depth tests and the
seed test, of the confidence threshold on either side of a pair, of the coverage threshold; ties, a pair with b1 > b2, the early end
and 32 sensors in ct_pair_kernel; d1 == 0 as a sample and not as coverage; every residue of ct_fold_kernel's unrolled loop, its sample
counts 0, 1, 7, 8, 9, 15, 16, 17; the projection's truncation, frame edges, infinities, NaN and clamp; the confidence pass's tile
borders, frame borders, frame sizes around its 32-pixel tile and its cap."""
import functools
import os

import numpy as np
import pytest

from livescan3d_amd import native
from tests import color_boundary_cases as cases, color_ref
from tests.support import PATTERN, Guarded, export

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "color_boundary_ref.npz")

_refs = {}


def _ref(orc, name):
    """color_ref.color_transfer of a rig: computed once, never changed."""
    if name not in _refs:
        v, d = color_ref.color_transfer(cases.rig(name), orc)
        for a in (v, d["confidence"], d["coverage"], d["transforms"]):
            a.setflags(write=False)
        _refs[name] = v, d
    return _refs[name]


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(GOLDEN)


def _same_diagnostics(got, want, what):
    assert np.array_equal(got["confidence"], want["confidence"]), (what, "confidence", int((got["confidence"] != want["confidence"]).sum()))
    assert np.array_equal(got["coverage"], want["coverage"]), (what, "coverage", got["coverage"].tolist())
    assert got["pairs"] == [tuple(p) for p in want["pairs"]], (what, got["pairs"], want["pairs"])
    assert got["transforms"].tobytes() == np.ascontiguousarray(want["transforms"], dtype=np.float64).tobytes(), (what, "transforms")


class Colour:
    """A plan of the rigs' sizes whose vertex buffer lies between guard bands: run_mesh, then the colour transfer."""

    def __init__(self, rigs):
        import torch
        from livescan3d_amd.fusion import DeviceFusion
        self.torch = torch
        self.fus = DeviceFusion.from_rigs(rigs)
        self.T, self.cap = self.fus.n_ticks, self.fus.capacity
        self.guard = Guarded(torch, self.T * self.cap * 16, self.fus.device)
        self.fus.vertices = self.guard.body().view(self.T, self.cap, 16)

    def load(self, rigs):
        """Other frames with their calibration into the same plan."""
        from livescan3d_amd.fusion import upload_rigs
        self.fus.set_params(rigs[0].intr, rigs[0].wt, rigs[0].bounds)
        self.fus.depth, self.fus.rgb = upload_rigs(rigs, self.T, self.fus.device.index)

    def run(self, between=None):
        self.guard.body().fill_(PATTERN)
        self.fus.run_mesh()
        if between is not None:
            between(self)
        self.before = self.fus.vertices.clone()
        self.fus.color_transfer()
        self.torch.cuda.synchronize()
        assert self.guard.intact(), "the colour transfer wrote outside the vertex buffer"
        return self

    def tick(self, k):
        """(vertex bytes (n, 16), whether the transfer left everything but the colour bytes of those vertices as it was)."""
        n = int(self.fus.host_offsets()[k, -1])
        slot, before = self.fus.vertices[k].cpu().numpy(), self.before[k].cpu().numpy()
        return slot[:n], slot[:n, 3:].tobytes() == before[:n, 3:].tobytes() and slot[n:].tobytes() == before[n:].tobytes()

    def check_tick(self, k, want, diag, what):
        got, rest_kept = self.tick(k)
        assert got.tobytes() == want.tobytes(), (what, len(got), len(want))
        assert rest_kept, (what, "A, XYZ or bytes behind the tick's vertices were written")
        _same_diagnostics(self.fus.plan.color_diagnostics(k), diag, what)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.fus.close()


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_export_equals_the_reference(gpu, orc, name):
    rig = cases.rig(name)
    want, diag = _ref(orc, name)
    plain, t0, e0 = export(rig)
    got, t1, e1 = export(rig, color_transfer=True)
    assert e0 == "" and e1 == "", (e0, e1)
    assert got.tobytes() == want.tobytes(), name
    if name not in cases.DEFINED:
        assert cases.equals_fixture(_fixture(), name, got), name          # the reference's own bytes, with nothing in between
    a, b = got.view(np.uint8).reshape(-1, 16), plain.view(np.uint8).reshape(-1, 16)
    assert a[:, 3:].tobytes() == b[:, 3:].tobytes() and t1.tobytes() == t0.tobytes()      # A, XYZ and the triangles are untouched
    assert (got.tobytes() != plain.tobytes()) == (bool(diag["pairs"]) and name != "ns_0")


@pytest.mark.parametrize("name", cases.NAMES)
def test_device_path_equals_the_reference(gpu, orc, name):
    want, diag = _ref(orc, name)
    with Colour([cases.rig(name)]) as c:
        c.run().check_tick(0, want, diag, name)


def test_ticks_of_one_plan(gpu, orc):
    """The tail rigs (sample counts 101 .. 108: every residue mod 8), cov_100 and rigs with other confidence maps as the ticks of one
    plan: blockIdx strides and per-tick slots of every kernel, and lsnFusionColorDiagnostics at ticks above 0 -- every tick equals the
    reference and its own single call, and no tick reports another's diagnostics."""
    ticks = [cases.rig(n) for n in cases.TICKS]
    for r in ticks:
        assert np.array_equal(r.intr, ticks[0].intr) and np.array_equal(r.wt, ticks[0].wt) and np.array_equal(r.bounds, ticks[0].bounds)
    assert set(cases.TAIL) < set(cases.TICKS) and cases.TICKS[0] in cases.TAIL
    with Colour(ticks) as c:
        c.run()
        batch = []
        for k, name in enumerate(cases.TICKS):
            c.check_tick(k, *_ref(orc, name), (k, name))
            batch.append((c.tick(k)[0].copy(), c.fus.plan.color_diagnostics(k)))
    first = batch[0][1]
    for k in range(1, len(batch)):
        d = batch[k][1]
        assert d["transforms"].tobytes() != first["transforms"].tobytes() and not np.array_equal(d["coverage"], first["coverage"]), k
    with Colour([ticks[0]]) as one:
        for k, name in enumerate(cases.TICKS):
            one.load([ticks[k]])
            one.run()
            assert one.tick(0)[0].tobytes() == batch[k][0].tobytes(), (k, name)
            _same_diagnostics(one.fus.plan.color_diagnostics(0), batch[k][1], (k, name))


def test_empty_sample_set(gpu, orc):
    """ns_0: the pair is chosen, every pixel of sensor 0 in the overlap has depth and none a vertex: ct_fold_kernel's ns == 0 branch."""
    rig = cases.rig("ns_0")
    plain, _, _ = export(rig)
    got, _, err = export(rig, color_transfer=True)
    assert err == "" and got.tobytes() == plain.tobytes()
    with Colour([rig]) as c:
        d = c.run().fus.plan.color_diagnostics(0)
        assert d["pairs"] == [(0, 1)] and d["transforms"].tolist() == [[0.0] * 6 + [1.0] * 3]
        assert c.tick(0)[0].tobytes() == plain.tobytes()


def test_small_sample_counts_on_one_plan(gpu, orc):
    """The ns_K rigs one after the other on one plan (one calibration, one crop box): 17 samples, then 0, then 9 ...: nothing of a
    call's samples, sums or transforms is left for the next."""
    order = ("ns_17", "ns_0", "ns_9", "ns_1", "ns_16", "ns_7", "ns_8", "ns_15", "ns_0")
    with Colour([cases.rig(order[0])]) as c:
        for name in order:
            c.load([cases.rig(name)])
            c.run().check_tick(0, *_ref(orc, name), name)


def test_32_sensors(gpu, orc):
    want, diag = _ref(orc, "n32")
    with Colour([cases.rig("n32")]) as c:
        d = c.run().fus.plan.color_diagnostics(0)
        off = c.fus.host_offsets()[0]
        got = c.tick(0)[0]
    assert len(d["pairs"]) == 31 and d["pairs"] == diag["pairs"]
    for i, j in d["pairs"]:      # every sensor's target: sensor j carries the transform of its own pair, the first pair's base none
        assert got[off[j]:off[j + 1]].tobytes() == want.view(np.uint8).reshape(-1, 16)[off[j]:off[j + 1]].tobytes(), (i, j)
    root = d["pairs"][0][0]
    plain, _, _ = export(cases.rig("n32"))
    assert got[off[root]:off[root + 1]].tobytes() == plain.view(np.uint8).reshape(-1, 16)[off[root]:off[root + 1]].tobytes()
    assert got.tobytes() == want.tobytes()


def _rig33():
    n, w, h = 33, 16, 8
    rng = np.random.default_rng(33)
    from livescan3d_amd import synth
    return synth.Rig([np.full((h, w), cases.L0, np.uint16)] * n, [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)],
                     np.tile(np.float32([w // 2, h // 2, 50, 50, 0, 0, 0]), n), np.tile(np.float32([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]), n), cases.WIDE)


def test_33_sensors_are_refused(gpu):
    """lsnFusionColorTransfer: -1 with a message that names the limit, and no byte of the vertices touched.  The export as it is today:
    the call with the flag fails as a whole -- an empty mesh and the same message -- while the call without it returns all 33 sensors."""
    rig = _rig33()
    with Colour([rig]) as c:
        c.guard.body().fill_(PATTERN)
        c.fus.run_mesh()
        c.torch.cuda.synchronize()
        before = c.guard.buf.clone()
        with pytest.raises(native.NativeUtilsError, match=r"lsnFusionColorTransfer: at most 32 sensors \(the plan has 33\)"):
            c.fus.color_transfer()
        c.torch.cuda.synchronize()
        assert bool((c.guard.buf == before).all().item()) and c.guard.intact()
    plain, _, e0 = export(rig)
    assert e0 == "" and len(plain) == 33 * 16 * 8
    with pytest.raises(native.NativeUtilsError, match=r"at most 32 sensors \(the plan has 33\)"):
        export(rig, color_transfer=True)
    again, _, e1 = export(rig)      # the failed call leaves the next one alone
    assert e1 == "" and again.tobytes() == plain.tobytes()


@pytest.mark.parametrize("name", ("cov_103", "b1_gt_b2"))
def test_alpha_other_than_255_is_kept(gpu, orc, name):
    """The export always hands the transfer A = 255; on the device path the caller's alpha bytes, whatever they are, stay."""
    want, diag = _ref(orc, name)
    alpha = (np.arange(len(want)) * 7 % 256).astype(np.uint8)
    assert (alpha != 255).sum() > len(want) // 2

    def set_alpha(c):
        n = int(c.fus.host_offsets()[0, -1])
        assert n == len(want)
        c.fus.vertices[0, :n, 3] = c.torch.from_numpy(alpha).to(c.fus.device)

    expect = want.copy()
    expect["A"] = alpha
    with Colour([cases.rig(name)]) as c:
        c.run(between=set_alpha).check_tick(0, expect, diag, name)
