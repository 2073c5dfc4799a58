"""Hand-made cases of depth smoothing (tests/depth_smooth_ref.py): each is named for what it reaches, carries a CPU witness that it does
reach it (`witness()` asserts), and lists the mutants of the restatement it must tell from the filter (`kills`).  The GPU tests run
every case through the kernels; tests/test_depth_smooth_ref.py runs the witnesses and the mutants without a device.
Also the seeded noisy frames the GPU tests share."""
import numpy as np

from tests import depth_smooth_ref as ref


class Case:
    def __init__(self, name, depth, r, ws, wr, kills=(), witness=None):
        self.name, self.r, self.kills, self._witness = name, r, tuple(kills), witness
        self.depth = np.asarray(depth, dtype=np.uint16)
        side = 2 * r + 1
        self.ws = np.asarray(ws, dtype=np.uint16).reshape(side, side)
        self.wr = np.asarray(wr, dtype=np.uint16).ravel()

    def want(self, mutant=None):
        return ref.smooth(self.depth, self.r, self.ws, self.wr, mutant)

    def witness(self):
        self._witness(self, self.want())


def _ones(r):
    return np.ones((2 * r + 1, 2 * r + 1), dtype=np.uint16)


def _w_halves(c, out):
    # pixel 0: W = 2, S = +1 -> (2 + 2) / 4 = 1 exactly a half above: up.  pixel 1: W = 2, S = -1 -> (-2 + 2) / 4 = 0: the half stays.
    W, S = ref.sums(c.depth, c.r, c.ws, c.wr)
    assert W.tolist() == [[2, 2]] and S.tolist() == [[1, -1]]
    assert out.tolist() == [[11, 11]]


def _w_negative_floor(c, out):
    # pixel 0: W = 2, S = -2 -> (-4 + 2) / 4 = -1/2: floor gives -1 (an exact half towards +infinity), truncation 0
    W, S = ref.sums(c.depth, c.r, c.ws, c.wr)
    assert (int(W[0, 0]), int(S[0, 0])) == (2, -2) and out[0, 0] == 11


def _w_range_cut(c, out):
    n = c.wr.size
    assert int(c.depth[0, 1]) - int(c.depth[0, 0]) == n - 1 and int(c.depth[0, 5]) - int(c.depth[0, 4]) == n
    assert out[0, 0] != c.depth[0, 0]                       # |delta| = n_range - 1 contributes
    assert out[0, 4] == c.depth[0, 4] and out[0, 5] == c.depth[0, 5]   # |delta| = n_range does not


def _w_zero_centre(c, out):
    assert c.depth[1, 1] == 0 and (np.delete(c.depth.ravel(), 4) != 0).all() and out[1, 1] == 0
    assert np.array_equal(out, c.depth)                     # the ring is constant: a fixed point, the hole is not filled


def _w_lonely(c, out):
    assert (c.depth != 0).sum() == 1 and np.array_equal(out, c.depth)


def _w_extremes(c, out):
    assert c.depth.min() == 0 and 1 in c.depth and 65535 in c.depth
    assert out[0, 1] == 1 and c.depth[0, 1] == 2            # a mean that comes down to 1
    assert out[2, 1] == 65535 and c.depth[2, 1] == 65534    # ... and one that comes up to 65535


def _w_big_sum(c, out):
    W, S = ref.sums(c.depth, c.r, c.ws, c.wr)
    assert S.max() > 2 ** 39 and S.min() < -(2 ** 39) and W.max() == 49 * 4095 * 4095 < 2 ** 30
    assert int(S[3, 3]) == 48 * 4095 * 4095 * 1023 and int(S[3, 13]) == -48 * 4095 * 4095 * 1023
    assert out[3, 3] == 1000 + 1002 and out[3, 13] == 2023 - 1002


def _w_asymmetric(c, out):
    assert not np.array_equal(c.ws, c.ws.T) and not np.array_equal(c.ws, c.ws[::-1]) and not np.array_equal(c.ws, c.ws[:, ::-1])
    for other in (c.ws.T, c.ws[::-1], c.ws[:, ::-1], c.ws[::-1, ::-1]):
        assert not np.array_equal(ref.smooth(c.depth, c.r, other, c.wr), out)


def _w_zero_entries(c, out):
    assert (c.ws == 0).sum() == 4 and (c.wr == 0).sum() == 1
    assert not np.array_equal(ref.smooth(c.depth, c.r, np.maximum(c.ws, 1), c.wr), out)     # the spatial zeros matter
    assert not np.array_equal(ref.smooth(c.depth, c.r, c.ws, np.maximum(c.wr, 1)), out)     # ... and so does the range table's


def _varied(h, w, seed, spread):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return (1500 + 4 * xx + 3 * yy + rng.integers(-spread, spread + 1, size=(h, w))).astype(np.uint16)


def _big_sum_depth():
    d = np.zeros((7, 17), dtype=np.uint16)
    d[:, 0:7] = 2023
    d[3, 3] = 1000          # 48 neighbours at +1023
    d[:, 10:17] = 1000
    d[3, 13] = 2023         # 48 neighbours at -1023
    return d


def cases():
    falling = np.array([4095, 3900, 3300, 2500, 1700, 1000, 500, 200, 60, 10, 1], dtype=np.uint16)
    return [
        Case("halves", [[10, 11]], 1, _ones(1), [1, 1, 1, 1], kills=("half_away", "oob_sample"), witness=_w_halves),
        Case("negative_floor", [[12, 10, 10]], 1, [[0, 0, 0], [0, 1, 1], [0, 0, 0]], [1, 1, 1, 1], kills=("trunc_div",), witness=_w_negative_floor),
        Case("range_cut", [[100, 104, 0, 0, 100, 105]], 1, _ones(1), [1, 0, 0, 0, 3], kills=("le_cut",), witness=_w_range_cut),
        Case("zero_centre", [[300, 300, 300], [300, 0, 300], [300, 300, 300]], 1, _ones(1), np.ones(1024), kills=("zero_neighbours",),
             witness=_w_zero_centre),
        Case("lonely", [[0, 0, 0], [0, 777, 0], [0, 0, 0]], 1, _ones(1), np.ones(1024), kills=("zero_neighbours",), witness=_w_lonely),
        Case("extremes", [[1, 2, 1], [0, 0, 0], [65535, 65534, 65535]], 1, _ones(1), [1, 1, 1, 1], kills=("zero_neighbours",), witness=_w_extremes),
        Case("big_sum", _big_sum_depth(), 3, np.full((7, 7), 4095), np.full(1024, 4095), kills=("s32",), witness=_w_big_sum),
        Case("asymmetric", _varied(6, 7, 5, 9), 1, [[1, 50, 300], [7, 4095, 900], [2000, 20, 120]], falling, kills=("transposed",),
             witness=_w_asymmetric),
        Case("asymmetric_r2", _varied(9, 11, 6, 9), 2, np.arange(1, 26) * 150, falling, kills=("transposed",), witness=_w_asymmetric),
        Case("zero_entries", _varied(5, 9, 7, 2), 1, [[0, 9, 0], [4, 1, 6], [0, 2, 0]], [5, 3, 0, 2], witness=_w_zero_entries),
    ]


def frame(seed, w, h):
    """A seeded noisy frame [h, w] u16: a sloped surface with a step, a few millimetres of noise, holes and a stripe near 65535."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = 1200 + 2 * xx + 3 * yy + 150 * ((xx // 19 + yy // 7) % 2) + rng.integers(-6, 7, size=(h, w))
    d[rng.random((h, w)) < 0.08] = 0
    if h > 2:
        d[h // 2, :] = 65535 - rng.integers(0, 9, size=w)
    return d.astype(np.uint16)


def random_tables(rng, r):
    """Valid random tables of radius r: (ws [2r+1, 2r+1], wr [n_range]) with zeros in both, n_range anywhere in 1..1024."""
    side = 2 * r + 1
    ws = rng.integers(0, 4096, size=(side, side))
    ws[rng.random((side, side)) < 0.2] = 0
    ws[r, r] = int(rng.integers(1, 4096))
    n = int(rng.choice([1, 2, 7, 40, 300, 1024, int(rng.integers(1, 1025))]))
    wr = rng.integers(0, 4096, size=n)
    wr[rng.random(n) < 0.2] = 0
    wr[0] = int(rng.integers(1, 4096))
    return ws.astype(np.uint16), wr.astype(np.uint16)
