"""Background subtraction (background.hip: lsnFusionSetBackground / lsnFusionBackgroundLearn / lsnFusionBackground / lsnFusionBackgroundReset /
lsnFusionBackgroundModelRead / lsnFusionBackgroundModelWrite / lsnFusionBackgroundDiagnostics) on the GPU.

Bar: bit for bit against the numpy restatement (tests/background_ref.py), for the maps AND the model; the diagnostics equal the
restatement's six counts per sensor and tick.  Every map buffer sits between guard bands.  Every test here fails on a library without the
feature (the exports do not exist)."""
import numpy as np
import pytest

from livescan3d_amd import native
from tests import background_cases as cases, background_ref as ref
from tests.support import Guarded

pytestmark = pytest.mark.gpu


class Batch:
    """A plan of `sizes` sensors and T ticks, its input at `shift` bytes behind a 16-byte boundary, input and output between guard bands."""

    def __init__(self, sizes, T, shift=0):
        import torch
        self.torch, self.sizes, self.T = torch, sizes, T
        self.widths, self.heights = [s[0] for s in sizes], [s[1] for s in sizes]
        self.plan = native.FusionPlan(0, T, self.widths, self.heights)
        self.px = self.plan.capacity
        assert self.px == sum(w * h for w, h in sizes)
        self.nbytes = 2 * self.px * T
        self.src = Guarded(torch, self.nbytes + shift, "cuda")
        self.dst = Guarded(torch, self.nbytes + shift, "cuda")
        self.src_ptr, self.dst_ptr, self.shift = self.src.ptr + shift, self.dst.ptr + shift, shift

    def load(self, maps):
        assert maps.shape == (self.T, self.px)
        self.src.body()[self.shift:].copy_(self.torch.from_numpy(np.ascontiguousarray(maps, "<u2").view(np.uint8).ravel().copy()))

    def source(self):
        return self.src.body()[self.shift:].cpu().numpy().view("<u2").reshape(self.T, self.px)

    def learn(self, maps):
        """-> the model after the call."""
        self.load(maps)
        self.plan.background_learn(self.src_ptr)
        self.torch.cuda.synchronize()
        assert self.src.intact() and np.array_equal(self.source(), maps)      # a learning pass writes no maps
        return self.plan.background_model()

    def run(self, in_place=False):
        """-> the subtracted maps [T, pixels]."""
        if not in_place:
            self.dst.body().fill_(0x5A)
        self.plan.background(self.src_ptr, self.src_ptr if in_place else self.dst_ptr)
        self.torch.cuda.synchronize()
        assert self.dst.intact() and self.src.intact()
        out = self.src if in_place else self.dst
        return out.body()[self.shift:].cpu().numpy().view("<u2").reshape(self.T, self.px)

    def check(self, maps, model, params, what, in_place=False):
        """One call on `maps` against `model` (None: the plan's own): maps, model and diagnostics against the restatement."""
        if model is not None:
            self.plan.set_background_model(model)
        before = self.plan.background_model()
        self.load(maps)
        want, counts, _ = ref.run(maps, before, self.widths, self.heights, *params)
        got = self.run(in_place)
        assert np.array_equal(got, want), (what, int((got != want).sum()))
        assert np.array_equal(self.plan.background_model(), before), what     # classification never changes the model
        if not in_place:
            assert np.array_equal(self.source(), maps), what                  # the input stays as it was
        for t in range(self.T):
            d = self.plan.background_diagnostics(t)
            assert d.tolist() == counts[t].tolist(), (what, t, d.tolist(), counts[t].tolist())
        return want

    def close(self):
        self.plan.close()


CASES = cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_hand_made_cases(gpu, case):
    """ModelWrite -> lsnFusionBackground -> ModelRead and the diagnostics on every hand-made case, out of place and in place."""
    b = Batch(case.sizes, case.maps.shape[0])
    b.plan.set_background(*case.params)
    b.check(case.maps, case.model, case.params, case.name)
    b.check(case.maps, None, case.params, (case.name, "in place"), in_place=True)
    b.close()


RIGS = {
    "one_pixel": ([(1, 1)], 1, 0),
    "element_wise_7x5": ([(7, 5), (1, 1)], 3, 0),
    "one_tile_128x16": ([(128, 16)], 2, 0),
    "four_tiles_129x17": ([(129, 17)], 2, 0),
    "wide_136x40": ([(136, 40), (8, 1)], 2, 0),
    "three_sizes": ([(129, 17), (7, 5), (136, 40)], 3, 0),
    "shifted_136x40": ([(136, 40), (128, 16)], 2, 2),               # widths of the 16-byte form, pointers 2 bytes off: element-wise
}


def rig_maps(rng, sizes, T):
    """A room to learn from and ticks with subjects in front of it, per sensor cases.blobby_mask."""
    px = sum(w * h for w, h in sizes)
    room = cases.learn_maps(rng, px, 3)
    wall = ref.learn(np.zeros(px, np.uint16), room).astype(np.int64)
    maps = np.clip(wall[None, :] + rng.integers(-30, 31, (T, px)), 1, 65535) * (wall != 0)[None, :]
    maps = np.where(rng.random(maps.shape) < 0.03, rng.integers(1, 65536, maps.shape), maps)   # (some samples on unseen pixels too)
    at = 0
    for w, h in sizes:
        for t in range(T):
            m = cases.blobby_mask(rng, w, h).ravel()
            maps[t, at:at + w * h][m] = wall[at:at + w * h][m] // 2
        at += w * h
    return room, maps.astype(np.uint16)


@pytest.mark.parametrize("name", list(RIGS))
def test_frames_across_every_tile_and_chunk_edge(gpu, name):
    """Learn, then three calls with three settings (no blob pass, a small and a large min_pixels; rel_q 0, 8 and 255), the last in place."""
    sizes, T, shift = RIGS[name]
    b = Batch(sizes, T, shift)
    rng = np.random.default_rng(sum(map(ord, name)))
    room, maps = rig_maps(rng, sizes, T)
    model = np.zeros(b.px, np.uint16)
    for k in range(0, 3, T):                                        # the room's three ticks in calls of the plan's size
        part = room[k:k + T]
        part = np.concatenate([part, np.zeros((T - part.shape[0], b.px), np.uint16)])      # (an all-zero tick teaches nothing)
        model = ref.learn(model, part)
        assert np.array_equal(b.learn(part), model), name
    seen = np.zeros(6, np.int64)
    for params, in_place in (((30, 8, 0), False), ((4095, 0, 3), False), ((1, 255, 40), True)):
        b.plan.set_background(*params)
        seen += ref.run(maps, model, b.widths, b.heights, *params)[1].sum(axis=(0, 1))
        b.check(maps, None, params, (name, params), in_place=in_place)
    if b.px > 500:
        assert (seen > 0).all(), seen                               # not vacuous: every count moved
    b.close()


def test_kinect_frame_512x424_once(gpu):
    sizes = [(512, 424)]
    b = Batch(sizes, 1)
    rng = np.random.default_rng(512)
    room, maps = rig_maps(rng, sizes, 1)
    model = ref.learn(np.zeros(b.px, np.uint16), room)
    b.plan.set_background(40, 8, 50)
    want = b.check(maps, model, (40, 8, 50), "512x424")
    assert want.any() and (want != maps).any()
    b.close()


def test_learning_in_any_order_and_any_split(gpu):
    """Five ticks as one call, permuted, as 2 + 3 and as five calls of one tick: one model, the restatement's; all-zero ticks change nothing."""
    sizes = [(136, 17), (9, 5)]
    rng = np.random.default_rng(77)
    px = sum(w * h for w, h in sizes)
    maps = cases.learn_maps(rng, px, 5)
    want = ref.learn(np.zeros(px, np.uint16), maps)
    assert (want == 0).any() and (want > 65000).any() and (want < 10).any()
    models = []
    for order, split in ((np.arange(5), [5]), (rng.permutation(5), [5]), (np.arange(5), [2, 3]), (rng.permutation(5), [1] * 5)):
        model, t0, plans = np.zeros(px, np.uint16), 0, {}
        for n in split:
            b = plans.get(n) or plans.setdefault(n, Batch(sizes, n))
            b.plan.set_background_model(model)                      # a plan takes the model over from the one before
            model = b.learn(maps[order][t0:t0 + n])
            t0 += n
        again = b.learn(np.zeros((split[-1], px), np.uint16))
        models.append((model, again))
        for b in plans.values():
            b.close()
    for model, again in models:
        assert np.array_equal(model, want) and np.array_equal(again, want)


def test_off_copies_refusals_change_nothing_and_reset(gpu):
    import torch
    sizes = [(136, 17), (7, 5)]
    b = Batch(sizes, 2)
    plan, L = b.plan, native.lib()
    rng = np.random.default_rng(3)
    room, maps = rig_maps(rng, sizes, 2)
    b.load(maps)
    with pytest.raises(native.NativeUtilsError):
        plan.background_diagnostics(0)                              # nothing has run yet
    assert not plan.background_model().any()
    # off by default: the call copies (in place: nothing) and leaves the model alone
    assert np.array_equal(b.run(), maps) and np.array_equal(b.run(in_place=True), maps)
    assert not plan.background_model().any() and not plan.background_diagnostics(1).any()
    # ModelWrite accepts any map; ModelRead hands it back
    anything = rng.integers(0, 65536, b.px).astype(np.uint16)
    plan.set_background_model(anything)
    assert np.array_equal(plan.background_model(), anything)
    assert np.array_equal(b.run(), maps) and np.array_equal(plan.background_model(), anything)      # still off
    # never learned and on: every sample is unknown and kept
    plan.background_reset()
    assert not plan.background_model().any()
    setting = (30, 8, 4)
    plan.set_background(30, 8, 0)
    assert np.array_equal(b.check(maps, None, (30, 8, 0), "nothing learned"), maps)
    model = b.learn(room[:2])
    assert np.array_equal(model, ref.learn(np.zeros(b.px, np.uint16), room[:2]))
    # on; every refused setting leaves the previous one in force, and the model
    plan.set_background(*setting)
    b.check(maps, None, setting, "on")
    for bad in [(4096, 8, 4), (30, -1, 4), (30, 256, 4), (30, 8, -1), (30, 8, (1 << 24) + 1)]:
        assert L.lsnFusionSetBackground(plan._h, *bad) == -1 and "lsnFusionSetBackground" in native.last_error(), bad
        b.check(maps, None, setting, ("after the refused setting", bad))
    assert L.lsnFusionSetBackground(plan._h, 4095, 255, 1 << 24) == 0
    plan.set_background(*setting)
    # an output that partly overlaps the input is refused with nothing written; so is a null argument
    b.load(maps)
    before = b.src.buf.cpu().numpy().tobytes()
    for out in (b.src_ptr + 16, b.src_ptr + b.nbytes - 2, b.src_ptr - 2):
        with pytest.raises(native.NativeUtilsError, match="overlap"):
            plan.background(b.src_ptr, out)
    b.dst.body().fill_(0x5A)
    assert L.lsnFusionBackground(plan._h, None, b.dst_ptr, None) == -1 and L.lsnFusionBackground(plan._h, b.src_ptr, None, None) == -1
    assert L.lsnFusionBackgroundLearn(plan._h, None, None) == -1
    torch.cuda.synchronize()
    assert b.src.buf.cpu().numpy().tobytes() == before and bool((b.dst.body() == 0x5A).all().item())
    assert np.array_equal(plan.background_model(), model)
    # off keeps the model, on again uses it; a reset clears it
    plan.set_background(0)
    assert np.array_equal(b.run(), maps) and np.array_equal(plan.background_model(), model)
    plan.set_background(*setting)
    b.check(maps, None, setting, "on again")
    plan.background_reset()
    assert not plan.background_model().any()
    b.check(maps, None, setting, "after the reset")
    b.close()


def test_more_ticks_than_the_blob_pass_takes_at_once(gpu):
    """19 ticks: the blob pass labels 16 at a time, so the last three run in a second round on the same scratch."""
    sizes = [(136, 17)]
    b = Batch(sizes, 19)
    rng = np.random.default_rng(19)
    room, maps = rig_maps(rng, sizes, 19)
    b.plan.set_background(30, 8, 5)
    b.check(maps, ref.learn(np.zeros(b.px, np.uint16), room), (30, 8, 5), "19 ticks")
    b.close()
