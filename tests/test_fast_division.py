"""Exhaustive proof of the division-free depth conversion used by the HIP kernel (csrc/fusion.hip, depth_to_metres):
for EVERY u16 depth d the sequence  q0 = d*r ; e = fma(-q0, 1000, d) ; q = fma(e, r, q0)  with r = fl32(1/1000)
is bit-identical to the reference's  float(d) / 1000.0f  (src/NativeUtils/depthprocessing.cpp:149-150).
Exact rational arithmetic, no floating-point shortcuts."""
from fractions import Fraction

import numpy as np


def rn32(F):
    """Correct rounding of a Fraction to float32 (nearest, ties to even)."""
    if F == 0:
        return np.float32(0)
    c = np.float32(float(F))
    best = None
    for x in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        err = abs(Fraction(float(x)) - F)
        if best is None or err < best[0] or (err == best[0] and (int(x.view(np.uint32)) & 1) == 0):
            best = (err, x)
    return best[1]


def test_three_instruction_quotient_is_exact_for_every_u16_depth():
    r = np.float32(1.0) / np.float32(1000.0)
    assert int(r.view(np.uint32)) == 0x3A83126F            # the literal in fusion.hip
    R = Fraction(float(r))
    for d in range(1, 65536):
        D = Fraction(d)
        want = np.float32(d) / np.float32(1000.0)           # IEEE-754 division
        assert want == rn32(D / 1000)
        q0 = rn32(D * R)
        e = rn32(D - Fraction(float(q0)) * 1000)
        q = rn32(Fraction(float(q0)) + Fraction(float(e)) * R)
        assert q == want, d


def test_integer_triangle_threshold_equals_the_double_expression():
    """csrc/fusion.hip computes checkTriangleConstraints' depth_thr (src/NativeUtils/meshGenerator.cpp:26,
    (int)((v0+v1+v2) / 3.0 * 0.00272 + 7.273) in double) as (272 s + 2181900) / 300000 in integers: equal for every
    possible sum s of three u16 depths."""
    s = np.arange(0, 3 * 65535 + 1, dtype=np.int64)
    ref = np.floor(s.astype(np.float64) / 3.0 * 0.00272 + 7.273).astype(np.int64)   # truncation = floor (positive)
    assert np.array_equal((272 * s + 2181900) // 300000, ref)


def test_division_free_edge_test_equals_the_threshold_compare():
    """csrc/mesh.hip (edges_pass): `metric < (272 s + 2181900) / 300000` is evaluated as `18750 * metric <= 17 * s + 117618` in 32-bit
    unsigned arithmetic on 24-bit factors.  For every sum s of three u16 depths the largest metric the product form accepts is exactly
    threshold - 1 (both forms are monotone in the metric, so the boundary decides every metric), nothing overflows, and the factors fit
    v_mul_u32_u24's 24 bits for every metric an edge can have (|vA - vB| <= 65535 bounds the minimum of its three differences)."""
    s = np.arange(0, 3 * 65535 + 1, dtype=np.int64)
    thr = (272 * s + 2181900) // 300000
    rhs = 17 * s + 117618
    largest_accepted = rhs // 18750                       # max metric with 18750 * metric <= rhs
    assert np.array_equal(largest_accepted, thr - 1)
    assert int(rhs.max()) < 2 ** 32 and 18750 * 65535 < 2 ** 32
    assert 65535 < 2 ** 24 and 18750 < 2 ** 24 and int(s.max()) < 2 ** 24 and 17 < 2 ** 24
    # spot check of the two predicates themselves around the boundary and at the extremes
    for m in (0, 1, 7, 8, 184, 185, 186, 65535):
        assert np.array_equal(m < thr, 18750 * m <= rhs), m
    # max(m0, m1, m2) < thr  <=>  every metric < thr
    rng = np.random.default_rng(5)
    m3 = rng.integers(0, 260, size=(200000, 3))
    t = rng.integers(0, 3 * 65535 + 1, size=200000)
    th = (272 * t + 2181900) // 300000
    assert np.array_equal((m3 < th[:, None]).all(axis=1), 18750 * m3.max(axis=1) <= 17 * t + 117618)


# ---- the biased, wrapped form the kernel computes (csrc/mesh.hip: biased_depth, edge_metric_z, edges_pass_z) -------------------------

BIAS, INVALID, M32 = 1 << 17, 1 << 30, (1 << 32) - 1
THR_ADD_BIASED = (117618 - 51 * BIAS) & M32               # kThrAddBiased: negative, kept as its 32-bit wrap


def test_biased_wrapped_threshold_compare_equals_the_threshold_for_every_sum():
    """edges_pass_z: (18750 m) mod 2^32 <= (17 (s + 3 * 2^17) + (117618 - 51 * 2^17)) mod 2^32 on the sum of three BIASED depths.  For
    every sum s of three u16 depths the largest metric it accepts is thr(s) - 1 -- among the metrics an edge can have (a minimum of three
    differences is at most |vA - vB| <= 65535) the left side does not wrap and is monotone, so the boundary decides every metric -- and both
    operands of each __umul24 fit 24 bits."""
    s = np.arange(0, 3 * 65535 + 1, dtype=np.uint64)
    thr = ((272 * s + 2181900) // 300000).astype(np.int64)
    s_biased = s + 3 * BIAS
    assert int(s_biased.max()) == 589821 and int(s_biased.max()) < 2 ** 24 and 17 < 2 ** 24 and 18750 < 2 ** 24 and 65535 < 2 ** 24
    assert 18750 * 65535 <= M32                                          # the left side never wraps
    rhs = (17 * s_biased + THR_ADD_BIASED) & M32                         # the kernel's right side, wrapped
    assert np.array_equal(rhs, 17 * s + 117618)                          # ... is the true, unbiased value
    largest_accepted = (rhs // 18750).astype(np.int64)
    assert np.array_equal(largest_accepted, thr - 1)
    for m in (0, 1, 6, 7, 8, 184, 185, 186, 65535):                      # the predicate itself, wrapped on both sides
        assert np.array_equal((np.uint64(18750 * m) & M32) <= rhs, m < thr), m
    # one off in the constant, or < for <=, is a different predicate: this is what the GPU boundary frames must see
    on_boundary = 18750 * (thr - 1).astype(np.uint64) == rhs
    assert on_boundary.any() and (18750 * thr.astype(np.uint64) == rhs + 1).any()


def _edge_metric_z(vA, vB, beyondB, beyondA):
    """edge_metric_z on uint32 arrays, as the kernel computes it: z = depth | 2^17, a 0 probe -> 2^30, d = zB - zA wrapped,
    |zA - zB|, |(zB + d) - pB|, |(zA - d) - pA| as unsigned absolute differences (v_sad_u32), their minimum."""
    def sad(a, b):
        return np.where(a >= b, a - b, b - a).astype(np.uint32)
    zA, zB = (vA | BIAS).astype(np.uint32), (vB | BIAS).astype(np.uint32)
    pB = np.where(beyondB != 0, beyondB | BIAS, INVALID).astype(np.uint32)
    pA = np.where(beyondA != 0, beyondA | BIAS, INVALID).astype(np.uint32)
    d = zB - zA                                                          # uint32: wraps
    return np.minimum(sad(zA, zB), np.minimum(sad(zB + d, pB), sad(zA - d, pA)))


def test_biased_edge_metric_equals_the_minimum_of_the_three_differences():
    """On 1.2 million seeded (vA, vB, beyondB, beyondA) -- uniform, near-linear (so the probes' differences are small), with 0 probes and
    the extremes 1 and 65535 -- edge_metric_z is the minimum of the reference's three differences over the rules that can pass
    (a 0 probe's rule cannot, meshGenerator.cpp:42, :51), and an invalid probe is never that minimum: its difference exceeds every
    threshold by far."""
    rng = np.random.default_rng(20261018)
    n = 300000
    ext = np.array([1, 65535, 2, 65534], dtype=np.int64)
    blocks = []
    blocks.append(rng.integers(1, 65536, size=(n, 4)))                                            # uniform
    vA = rng.integers(1, 65536, size=n)
    vB = np.clip(vA + rng.integers(-400, 401, size=n), 1, 65535)
    blocks.append(np.stack([vA, vB, np.clip(2 * vB - vA + rng.integers(-200, 201, size=n), 1, 65535),
                            np.clip(2 * vA - vB + rng.integers(-200, 201, size=n), 1, 65535)], axis=1))   # near-linear
    blocks.append(ext[rng.integers(0, 4, size=(n, 4))])                                           # the extremes
    mixed = rng.integers(1, 65536, size=(n, 4))
    mixed[:, :2] = np.where(rng.random((n, 2)) < 0.3, ext[rng.integers(0, 4, size=(n, 2))], mixed[:, :2])
    blocks.append(mixed)
    t = np.concatenate(blocks)
    t[:, 2] = np.where(rng.random(len(t)) < 0.25, 0, t[:, 2])                                     # 0 probes: either, both
    t[:, 3] = np.where(rng.random(len(t)) < 0.25, 0, t[:, 3])
    assert len(t) >= 10 ** 6 and ((t[:, 2] == 0) & (t[:, 3] == 0)).any() and (t[:, :2] > 0).all()
    vA, vB, pB, pA = (t[:, k].astype(np.int64) for k in range(4))
    big = np.int64(1) << 40
    want = np.minimum(np.abs(vA - vB), np.minimum(np.where(pB != 0, np.abs(vB - vA - (pB - vB)), big),
                                                  np.where(pA != 0, np.abs(vB - vA - (vA - pA)), big)))
    got = _edge_metric_z(*(t[:, k].astype(np.uint32) for k in range(4)))
    assert np.array_equal(got.astype(np.int64), want)
    # an invalid probe's own difference: at least 2^30 - (2^17 + 3 * 65535), no threshold (<= 185) reaches it
    zA, zB = (vA | BIAS), (vB | BIAS)
    assert int(np.abs(2 * zB - zA - INVALID).min()) > 10 ** 9 and int(np.abs(2 * zA - zB - INVALID).min()) > 10 ** 9
    assert int(want.max()) <= 65535                                       # the metric's factor fits v_mul_u32_u24's 24 bits
