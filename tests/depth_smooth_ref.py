"""Numpy restatement of depth smoothing, the integer bilateral filter depth_smooth.hip implements (include/NativeUtils.h holds the
wording, DESIGN.md section 20 the layout).  The reference has no such step: this file IS the yardstick, and the kernels are held to it bit
for bit.  Everything is int64.

One u16 map D of w x h (millimetres, 0 = no sample), a radius r in {1, 2, 3}, a spatial table ws[(2r+1)^2] (row-major over (dy, dx)), a
range table wr[n_range] indexed by |delta|; entries <= 4095, 1 <= n_range <= 1024, ws[centre] >= 1, wr[0] >= 1.  Per pixel c = D[y][x]:
  * c == 0: out = 0;
  * otherwise a window position (dy, dx), |dy|, |dx| <= r, centre included, contributes iff it lies inside the frame, its value v != 0 and
    a = |v - c| < n_range; its weight is wt = ws[dy+r][dx+r] * wr[a];
  * W = sum wt, S = sum wt * (v - c), out = c + floor((2 S + W) / (2 W)) -- floor division: an exact half rounds towards +infinity.
Every decision reads the unmodified map.

`mutant` names a deliberately wrong variant (tests/test_depth_smooth_ref.py proves that the hand-made cases tell each from the filter):
  "oob_sample"      out-of-frame positions count, with the nearest in-frame pixel's value
  "zero_neighbours" neighbours of value 0 count like any other value
  "le_cut"          a <= n_range contributes (with the table's last entry at a == n_range)
  "trunc_div"       the division truncates towards zero
  "half_away"       an exact half rounds away from zero
  "s32"             S is kept in 32 bits (wraps)
  "transposed"      the spatial table is read column-major"""
import numpy as np

MUTANTS = ("oob_sample", "zero_neighbours", "le_cut", "trunc_div", "half_away", "s32", "transposed")


def tables(r, ws, wr):
    r = int(r)
    side = 2 * r + 1
    ws = np.asarray(ws, dtype=np.int64).reshape(side, side)
    wr = np.asarray(wr, dtype=np.int64).ravel()
    assert 1 <= r <= 3 and 1 <= wr.size <= 1024 and ws.max() <= 4095 and wr.max() <= 4095 and ws.min() >= 0 and wr.min() >= 0
    assert ws[r, r] >= 1 and wr[0] >= 1
    return r, ws, wr


def sums(depth, r, ws, wr, mutant=None):
    """(W, S) per pixel as int64 arrays [h, w] (whatever the centre's value)."""
    assert mutant is None or mutant in MUTANTS
    r, ws, wr = tables(r, ws, wr)
    if mutant == "transposed":
        ws = ws.T
    c = np.asarray(depth).astype(np.int64)
    assert c.ndim == 2
    h, w = c.shape
    n = wr.size
    if mutant == "oob_sample":
        P, inside = np.pad(c, r, mode="edge"), np.ones((h + 2 * r, w + 2 * r), dtype=bool)
    else:
        P, inside = np.pad(c, r), np.pad(np.ones((h, w), dtype=bool), r)
    W, S = np.zeros((h, w), dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            v = P[r + dy:r + dy + h, r + dx:r + dx + w]
            a = np.abs(v - c)
            on = inside[r + dy:r + dy + h, r + dx:r + dx + w] & (a <= n if mutant == "le_cut" else a < n)
            if mutant != "zero_neighbours":
                on = on & (v != 0)
            wt = ws[dy + r, dx + r] * wr[np.minimum(a, n - 1)] * on
            W += wt
            S += wt * (v - c)
    if mutant == "s32":
        S = ((S + 2 ** 31) % 2 ** 32) - 2 ** 31
    return W, S


def smooth(depth, r, ws, wr, mutant=None):
    """The smoothed map (a new u16 array [h, w])."""
    c = np.asarray(depth).astype(np.int64)
    W, S = sums(c, r, ws, wr, mutant)
    W = np.where(c == 0, 1, W)            # (a zero centre's sums mean nothing)
    num, den = 2 * S + W, 2 * W
    if mutant == "trunc_div":
        q = np.sign(num) * (np.abs(num) // den)
    elif mutant == "half_away":
        q = np.sign(S) * ((2 * np.abs(S) + W) // den)
    else:
        q = num // den                    # numpy's // on integers is floor division
    out = np.where(c == 0, 0, c + q)
    if mutant is None:
        assert out.min() >= 0 and out.max() <= 65535
    return (out & 0xFFFF).astype(np.uint16)


def counts(depth, out):
    """(pixels with out != in, sum of |out - in|): what lsnFusionDepthSmoothDiagnostics reports per sensor."""
    d = np.asarray(out).astype(np.int64) - np.asarray(depth).astype(np.int64)
    return int((d != 0).sum()), int(np.abs(d).sum())


def smooth_packed(depth_maps, widths, heights, r, ws, wr):
    """The filter on every frame of a call's packed depth array (uint8 view of little-endian u16).
    Returns (smoothed packed uint8 array, changed pixels per sensor int32, sum of |out - in| per sensor int64)."""
    dm = np.ascontiguousarray(depth_maps).view(np.uint8).view("<u2").copy()
    changed, moved, p = [], [], 0
    for w, h in zip(np.asarray(widths).tolist(), np.asarray(heights).tolist()):
        f = dm[p:p + w * h].reshape(h, w).copy()
        o = smooth(f, r, ws, wr)
        k, m = counts(f, o)
        changed.append(k)
        moved.append(m)
        dm[p:p + w * h] = o.ravel()
        p += w * h
    return dm.view(np.uint8), np.array(changed, dtype=np.int32), np.array(moved, dtype=np.int64)


def gaussian(radius, sigma_s, sigma_r, range_cap=1024):
    """lsnDepthSmoothGaussian in numpy (float32 sigmas widened to double, like the export's).  An entry may differ from the library's by
    one unit where two exp implementations differ in the last bit."""
    r = int(radius)
    ss, sr = float(np.float32(sigma_s)), float(np.float32(sigma_r))
    dy, dx = np.mgrid[-r:r + 1, -r:r + 1]
    ws = np.rint(4095.0 * np.exp(-(dx * dx + dy * dy).astype(np.float64) / (2.0 * ss * ss))).astype(np.int64)
    k = np.arange(min(int(range_cap), 1024), dtype=np.float64)
    wr = np.rint(4095.0 * np.exp(-(k * k) / (2.0 * sr * sr))).astype(np.int64)
    zero = np.flatnonzero(wr == 0)
    return ws, wr[:zero[0]] if zero.size else wr
