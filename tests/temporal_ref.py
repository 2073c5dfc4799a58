"""Numpy restatement of the temporal depth filter, the range-gated recursive mean across ticks that temporal.hip implements
(include/NativeUtils.h holds the wording, DESIGN.md section 22 the layout).  The reference has no such step: this file IS the yardstick, and
the kernel is held to it bit for bit, in maps and in state.  Everything is int64.

Per tick one u16 map D (millimetres, 0 = no sample) per sensor; parameters alpha_q in 1..256 (the new sample's weight in 1/256), delta in
1..4095 mm (the gate), persist in 0..255 (consecutive ticks a missing sample is served from history).  State: one u32 word per pixel,
F | miss << 24 -- F the filtered depth in 1/256 mm (0: no history, else 256 .. 65535 * 256), miss the consecutive ticks served from
history; the word 0 is "no history".  Per pixel and tick, with sample c:
  1. blend    c != 0, F != 0, |256 c - F| <= 256 delta:  F' = F + floor((alpha_q (256 c - F) + 128) / 256), miss' = 0,
              out = floor((F' + 128) / 256)
  2. restart  c != 0 otherwise (no history, or the gate failed):  F' = 256 c, miss' = 0, out = c
  3. fill     c == 0, F != 0, miss < persist:  F' = F, miss' = miss + 1, out = floor((F + 128) / 256)
  4. expire / empty  c == 0 otherwise:  the word becomes 0, out = 0
Ticks are sequential per pixel; the pass is pointwise.

`mutant` names a deliberately wrong variant (tests/test_temporal_ref.py proves that the hand-made cases tell each from the filter):
  "lt_gate"        the gate is |256 c - F| < 256 delta
  "trunc"          the blend's division truncates towards zero
  "no_half_blend"  the blend's division lacks the + 128
  "no_half_out"    the served value is floor(F / 256)
  "le_persist"     a fill needs miss <= persist
  "miss_kept"      a sample does not clear miss
  "state_kept"     a gate failure serves c but keeps the old state
  "out_c"          a blend serves c"""
import numpy as np

MUTANTS = ("lt_gate", "trunc", "no_half_blend", "no_half_out", "le_persist", "miss_kept", "state_kept", "out_c")

# what a pixel-tick did
EMPTY, BLEND, RESTART, START, FILL, EXPIRE = range(6)
BRANCHES = ("empty", "blend", "restart", "start", "fill", "expire")
F_MIN, F_MAX = 256, 65535 * 256


def params_ok(alpha_q, delta, persist):
    return 1 <= int(alpha_q) <= 256 and 1 <= int(delta) <= 4095 and 0 <= int(persist) <= 255


def state_ok(state):
    """What lsnFusionTemporalStateWrite admits: F in {0} u [256, 65535 * 256], and miss == 0 wherever F == 0."""
    s = np.asarray(state).astype(np.int64)
    F, miss = s & 0xFFFFFF, s >> 24
    return bool((((F == 0) & (miss == 0)) | ((F >= F_MIN) & (F <= F_MAX))).all())


def pack(F, miss=0):
    return (np.asarray(F).astype(np.int64) | (np.asarray(miss).astype(np.int64) << 24)).astype(np.uint32)


def step(depth, state, alpha_q, delta, persist, mutant=None):
    """One tick: (out u16, state' u32, branch uint8), each shaped like `depth`."""
    assert mutant is None or mutant in MUTANTS
    assert params_ok(alpha_q, delta, persist)
    a, dl, ps = int(alpha_q), int(delta), int(persist)
    c = np.asarray(depth).astype(np.int64)
    s = np.asarray(state).astype(np.int64)
    assert c.shape == s.shape and state_ok(s)
    F, miss = s & 0xFFFFFF, s >> 24
    diff = 256 * c - F
    gate = (np.abs(diff) < 256 * dl) if mutant == "lt_gate" else (np.abs(diff) <= 256 * dl)
    sample, hist = c != 0, F != 0
    blend = sample & hist & gate
    restart = sample & ~blend
    fill = ~sample & hist & ((miss <= ps) if mutant == "le_persist" else (miss < ps))
    drop = ~sample & ~fill

    num = a * diff + (0 if mutant == "no_half_blend" else 128)
    q = np.sign(num) * (np.abs(num) // 256) if mutant == "trunc" else num // 256   # numpy's // on integers is floor division
    Fb = F + q
    half = 0 if mutant == "no_half_out" else 128
    F2 = np.where(blend, Fb, np.where(restart, 256 * c, np.where(fill, F, 0)))
    m2 = np.where(fill, miss + 1, 0)
    if mutant == "miss_kept":
        m2 = np.where(sample, miss, m2)
    if mutant == "state_kept":
        keep = restart & hist
        F2, m2 = np.where(keep, F, F2), np.where(keep, miss, m2)
    out = np.where(blend, c if mutant == "out_c" else (Fb + half) // 256, np.where(restart, c, np.where(fill, (F + half) // 256, 0)))
    if mutant is None:
        # the header's consequences, on every call
        assert ((Fb >= np.minimum(F, 256 * c)) & (Fb <= np.maximum(F, 256 * c)))[blend].all()
        assert ((out >= 1) & (out <= 65535))[~drop].all() and (out[drop] == 0).all()
        assert (m2 <= 255).all() and ((F2 == 0) | ((F2 >= F_MIN) & (F2 <= F_MAX))).all()
    branch = np.where(blend, BLEND, np.where(restart & hist, RESTART, np.where(restart, START, np.where(fill, FILL, np.where(hist, EXPIRE, EMPTY)))))
    return (out & 0xFFFF).astype(np.uint16), ((F2 & 0xFFFFFF) | ((m2 & 0xFF) << 24)).astype(np.uint32), branch.astype(np.uint8)


def run(maps, state, alpha_q, delta, persist, mutant=None):
    """A call of len(maps) ticks: (out u16 [T, ...], state' u32, branch uint8 [T, ...])."""
    maps = np.asarray(maps)
    outs, brs = np.zeros(maps.shape, np.uint16), np.zeros(maps.shape, np.uint8)
    s = np.asarray(state).astype(np.uint32)
    for t in range(maps.shape[0]):
        outs[t], s, brs[t] = step(maps[t], s, alpha_q, delta, persist, mutant)
    return outs, s, brs


def counts(branch):
    """(blended, restarted with history, filled, expired): what lsnFusionTemporalDiagnostics reports per sensor and tick."""
    b = np.asarray(branch)
    return int((b == BLEND).sum()), int((b == RESTART).sum()), int((b == FILL).sum()), int((b == EXPIRE).sum())


def sensor_slices(widths, heights):
    p, out = 0, []
    for w, h in zip(np.asarray(widths).tolist(), np.asarray(heights).tolist()):
        out.append(slice(p, p + w * h))
        p += w * h
    return out


def run_packed(depth_maps, state, alpha_q, delta, persist):
    """One tick on a call's packed depth array (uint8 view of little-endian u16) with `state` u32 [pixels] (None: no history).
    Returns (filtered packed uint8 array, state')."""
    dm = np.ascontiguousarray(depth_maps).view(np.uint8).view("<u2")
    s = np.zeros(dm.size, np.uint32) if state is None else state
    out, s2, _ = step(dm, s, alpha_q, delta, persist)
    return out.astype("<u2").view(np.uint8), s2


def pixel(c, word, alpha_q, delta, persist):
    """The definition once more as a plain-Python loop body over one pixel: (out, word', branch).  Python's // is mathematical floor."""
    F, miss = word & 0xFFFFFF, word >> 24
    if c != 0:
        d = 256 * c - F
        if F != 0 and abs(d) <= 256 * delta:
            F2 = F + (alpha_q * d + 128) // 256
            return (F2 + 128) // 256, F2, BLEND
        return c, 256 * c, RESTART if F != 0 else START
    if F != 0 and miss < persist:
        return (F + 128) // 256, F | ((miss + 1) << 24), FILL
    return 0, 0, EXPIRE if F != 0 else EMPTY
