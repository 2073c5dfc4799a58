"""Hand-made sequences for the temporal depth filter (tests/temporal_ref.py restates it), and the generator of the fuzz tests' inputs.

A case is one row of pixels (w x 1) over T ticks with a seeded state (what lsnFusionTemporalStateWrite writes), so that a fractional F is
reachable in one tick.  Each carries a witness: a numpy check that the sequence reaches the branch or boundary it is named for."""
import numpy as np

from tests import temporal_ref as ref

B = ref  # the branch codes


class Case:
    def __init__(self, name, params, state, maps, witness):
        self.name, self.params = name, tuple(int(p) for p in params)
        self.state = np.asarray(state, dtype=np.uint32).ravel()
        self.maps = np.asarray(maps, dtype=np.uint16).reshape(-1, self.state.size)
        self._witness = witness

    def want(self, mutant=None):
        return ref.run(self.maps, self.state, *self.params, mutant=mutant)

    def witness(self):
        out, state, br = self.want()
        F0, m0 = self.state.astype(np.int64) & 0xFFFFFF, self.state.astype(np.int64) >> 24
        self._witness(self, out.astype(np.int64), state.astype(np.int64), br, F0, m0)


def _gate(delta):
    # |256 c - F| = 256 delta - 1, 256 delta, 256 delta + 1, the sample above and below the history
    c = 5000
    edge = 256 * delta
    diffs = [edge - 1, edge, edge + 1, -(edge - 1), -edge, -(edge + 1)]
    F = [256 * c - d for d in diffs]

    def witness(k, out, state, br, F0, m0):
        d = 256 * k.maps[0].astype(np.int64) - F0
        assert np.abs(d).tolist() == [edge - 1, edge, edge + 1] * 2
        assert br[0].tolist() == [B.BLEND, B.BLEND, B.RESTART] * 2
        assert (state[[2, 5]] == 256 * c).all() and (state[[0, 1, 3, 4]] != 256 * c).all()
    return Case(f"gate_delta_{delta}", (128, delta, 0), ref.pack(F), [[c] * 6], witness)


def _alpha(alpha):
    diffs = [1, -1, 255, -255, 300, -300, 5119, -5119, 5120, -5120]
    c = 3000
    F = [256 * c - d for d in diffs]

    def witness(k, out, state, br, F0, m0):
        assert (br[0] == B.BLEND).all()
        F2 = state & 0xFFFFFF
        if alpha == 256:
            assert (F2 == 256 * c).all() and (out[0] == c).all()
        else:
            assert (F2 != 256 * c).any() and (F2 != F0).any()
    return Case(f"alpha_{alpha}", (alpha, 20, 0), ref.pack(F), [[c] * len(diffs)], witness)


def _rounding():
    # alpha_q * diff + 128 one below, on and one above a multiple of 256, diff > 0 and diff < 0 (alpha_q = 3: 3 * 171 = 1 mod 256)
    alpha, c = 3, 4000
    diffs = []
    for sign in (1, -1):
        for r in (255, 0, 1):
            d = ((r - 128) * 171) % 256 + (1024 if sign > 0 else -2048)
            diffs.append(d)
    F = [256 * c - d for d in diffs]

    def witness(k, out, state, br, F0, m0):
        d = 256 * k.maps[0].astype(np.int64) - F0
        num = alpha * d + 128
        assert (num % 256).tolist() == [255, 0, 1] * 2 and (num[:3] > 0).all() and (num[3:] < 0).all()
        assert (br[0] == B.BLEND).all()
        trunc = np.sign(num) * (np.abs(num) // 256)
        assert (trunc[[3, 5]] != num[[3, 5]] // 256).all() and trunc[4] == num[4] // 256      # floor against truncation
        assert ((alpha * d) // 256 != num // 256).any()                                        # the half is placed
        F2 = state & 0xFFFFFF
        assert ((F2 % 256) >= 128).any() and ((F2 % 256) < 128).any()                          # ... in the served value too
    return Case("rounding_floor_and_half", (alpha, 20, 0), ref.pack(F), [[c] * 6], witness)


def _stall():
    c = 2000
    diffs = [127, -127, 128, -128, 129, -129]
    F = [256 * c - d for d in diffs]

    def witness(k, out, state, br, F0, m0):
        assert (br[0] == B.BLEND).all()
        moved = (state & 0xFFFFFF) - F0
        assert moved.tolist() == [0, 0, 1, 0, 1, -1]      # |alpha_q diff| < 128 stalls; -128 + 128 = 0 stalls too
    return Case("stall", (1, 20, 0), ref.pack(F), [[c] * 6], witness)


def _extremes():
    lo, hi = ref.F_MIN, ref.F_MAX
    #        blend at the ends         restart across the range   fill at the ends / fractional
    F = [lo, lo, hi, hi, lo + 127, hi, lo, lo, hi, lo + 127, lo + 128, hi - 129]
    c = [1, 2, 65535, 65534, 1, 1, 65535, 0, 0, 0, 0, 0]

    def witness(k, out, state, br, F0, m0):
        assert br[0].tolist() == [B.BLEND] * 5 + [B.RESTART] * 2 + [B.FILL] * 5
        assert out[0].min() == 1 and out[0].max() == 65535
        assert out[0, 7:].tolist() == [1, 65535, 1, 2, 65534]
        assert (state[[5, 6]] == [256, 65535 * 256]).all()
    return Case("extremes_of_F_and_c", (128, 4095, 1), ref.pack(F), [c], witness)


def _persist():
    # (persist, miss) pairs at persist - 1 and persist, one case per persist; and a miss above persist (a setting lowered over a history)
    cases = []
    for persist, misses, want in [(0, [0, 3], [B.EXPIRE, B.EXPIRE]), (1, [0, 1, 7], [B.FILL, B.EXPIRE, B.EXPIRE]),
                                  (255, [254, 255, 0], [B.FILL, B.EXPIRE, B.FILL])]:
        F = [256 * 1500 + 77] * len(misses)

        def witness(k, out, state, br, F0, m0, want=want, misses=misses, persist=persist):
            assert br[0].tolist() == want
            for i, b in enumerate(want):
                assert state[i] == (0 if b == B.EXPIRE else (256 * 1500 + 77) | ((misses[i] + 1) << 24))
                assert out[0, i] == (0 if b == B.EXPIRE else 1500)
            if persist == 255:
                assert (state[0] >> 24) == 255                     # miss goes from 254 to 255
        cases.append(Case(f"persist_{persist}", (64, 20, persist), ref.pack(F, misses), [[0] * len(misses)], witness))

    def witness255(k, out, state, br, F0, m0):
        assert br[:, 0].tolist() == [B.FILL, B.EXPIRE, B.EMPTY] and state[0] == 0
    cases.append(Case("miss_254_255_then_expires", (64, 20, 255), ref.pack([256 * 900], [254]), [[0], [0], [0]], witness255))
    return cases


def _hole_without_history():
    def witness(k, out, state, br, F0, m0):
        assert (br == B.EMPTY).all() and (state == 0).all() and (out == 0).all()
    return Case("hole_without_history", (64, 20, 2), [0, 0], [[0, 0], [0, 0]], witness)


def _return_after_fill():
    # start, a fill, then the sample comes back inside the gate (pixel 0), on its edge (1) and outside it (2)
    maps = [[1000, 1000, 1000], [0, 0, 0], [1010, 1020, 1021]]

    def witness(k, out, state, br, F0, m0):
        assert br[:, 0].tolist() == [B.START, B.FILL, B.BLEND] and br[2].tolist() == [B.BLEND, B.BLEND, B.RESTART]
        _, mid, _ = ref.run(k.maps[:2], k.state, *k.params)
        assert (mid.astype(np.int64) >> 24).tolist() == [1, 1, 1] and (state >> 24).tolist() == [0, 0, 0]     # the sample clears miss
        assert out[1].tolist() == [1000] * 3 and out[2, 0] not in (1000, 1010)
    return Case("sample_returns_after_a_fill", (64, 20, 2), [0, 0, 0], maps, witness)


def _reblend_after_gate_failure():
    maps = [[1000], [2000], [2003]]

    def witness(k, out, state, br, F0, m0):
        assert br[:, 0].tolist() == [B.BLEND, B.RESTART, B.BLEND]
        assert out[1, 0] == 2000 and (state[0] & 0xFFFFFF) == 2000 * 256 + 3 * 128 and out[2, 0] == 2002     # (2001.5 rounds up)
    return Case("gate_failure_then_reblend", (128, 20, 0), ref.pack([256 * 1001 + 13]), maps, witness)


def cases():
    out = [_gate(d) for d in (1, 20, 4095)] + [_alpha(a) for a in (1, 255, 256)]
    out += [_rounding(), _stall(), _extremes()] + _persist()
    out += [_hole_without_history(), _return_after_fill(), _reblend_after_gate_failure()]
    return out


# ---- the fuzz tests' inputs -------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = tuple(range(12))
ALPHAS, DELTAS, PERSISTS = (1, 26, 64, 128, 255, 256), (1, 8, 20, 40, 4095), (0, 1, 2)


def fuzz_params(rng):
    """(alpha_q, delta, persist): the extremes of alpha_q and delta among them, persist from {0, 1, 2}."""
    return int(rng.choice(ALPHAS)), int(rng.choice(DELTAS)), int(rng.choice(PERSISTS))


def fuzz_maps(rng, n_pixels, n_ticks):
    """[n_ticks, n_pixels] u16: a per-pixel base, noise of a few millimetres, random jumps of the base (motion, edges), about 25 %
    dropouts, a tenth of the pixels dead for good."""
    base = rng.integers(400, 8000, n_pixels).astype(np.int64)
    dead = rng.random(n_pixels) < 0.10
    maps = np.zeros((n_ticks, n_pixels), np.uint16)
    for t in range(n_ticks):
        jump = rng.random(n_pixels) < 0.12
        base = np.where(jump, rng.integers(400, 8000, n_pixels), base)
        v = base + rng.integers(-4, 5, n_pixels)
        drop = dead | (rng.random(n_pixels) < 0.25)
        maps[t] = np.where(drop, 0, v)
    return maps


def fuzz_case(seed):
    """The seed's (sizes [(w, h)], params, maps [n_ticks, pixels]): 1..3 sensors of support.ring_rig's sizes, 2..9 ticks."""
    from tests import support
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(1, 4))
    sizes = support.ragged_or_equal(140, 20, [8, 128, 136], [1, 16, 17])(rng, n)
    params = fuzz_params(rng)
    n_ticks = int(rng.integers(2, 10))
    return sizes, params, fuzz_maps(rng, sum(w * h for w, h in sizes), n_ticks)
