"""Hand-made clouds for the outlier filter (csrc/outlier.hip) at its decision boundaries, each with a witness.

A Case holds a name, the frame sizes of its plan (they fix the bucket tables: max(64, the power of two >= w * h) buckets per sensor), a
per-tick list of per-sensor (n, 3) float32 blocks, (k, maxDist) and a witness: an assertion, on the restatement's own result
(tests/outlier_ref.py) and on the grid restated below, that the case reaches what it is named for and that the named thing decides a
vertex.  All coordinates are finite.

The grid restated (edge, corner, cell, ol_hash, the order of the 27 cells) serves the witnesses alone: it shows that a case reaches a
situation of the grid, and is never an expected value.  Should the kernel's constants change, the witnesses fail and say so.

tests/test_outlier_boundary_ref.py runs the witnesses, holds the restatement to the reference's own filter() on every block
(tests/golden/outlier_boundary_ref.npz) and tells every wrong rule of outlier_ref.RULES apart by the cases of KILLS;
tests/test_outlier_boundary_gpu.py runs the cases through lsnFusionOutlierFilter."""
import functools
import itertools

import numpy as np

from tests import outlier_ref as ref

F = np.float32
MIN_BUCKETS = 64
FRAME_64 = (8, 8)        # 64 pixels: the smallest table
FRAME_POW2 = (64, 1)     # exactly a power of two
FRAME_PAST = (65, 1)     # one past it: 128 buckets
FRAME_4096 = (64, 64)


class Case:
    def __init__(self, name, frames, ticks, k, max_dist, witness, note=""):
        self.name, self.frames, self.k, self.max_dist, self.witness, self.note = name, list(frames), int(k), F(max_dist), witness, note
        self.ticks = [[np.ascontiguousarray(np.asarray(b, dtype=F).reshape(-1, 3)) for b in tick] for tick in ticks]
        assert all(len(t) == len(self.frames) for t in self.ticks), name
        assert all(np.isfinite(b).all() for t in self.ticks for b in t), name
        assert max(sum(len(b) for b in t) for t in self.ticks) <= sum(w * h for w, h in self.frames), name   # a tick's capacity

    def blocks(self):
        """(tick, sensor, points) of every block, in the fixture's order."""
        return [(t, s, b) for t, tick in enumerate(self.ticks) for s, b in enumerate(tick)]

    def keep(self, rules=None, brute_limit=8000):
        return ref.filter_batch(self.ticks, self.k, self.max_dist, rules=rules, brute_limit=brute_limit)

    def counts(self):
        """Per tick: (removed per sensor, vertices the grid pass decided per sensor), as lsnFusionOutlierDiagnostics reports them."""
        on = self.k > 0 and self.max_dist > 0
        return [([int((~m).sum()) for m in row], [len(m) if on and len(m) >= self.k else 0 for m in row]) for row in self.keep()]


# ---- the grid, restated ----------------------------------------------------------------------------------------------------------

def buckets_of(frame):
    b = MIN_BUCKETS
    while b < frame[0] * frame[1]:
        b <<= 1
    return b


def edge0(max_dist):
    return float(F(max_dist)) * (1.0 + 2.0 ** -20) + 2.0 ** -70


class Grid:
    """The grid of one block: corner, edge (e0 unless `edge` is given), cells, buckets."""

    def __init__(self, block, max_dist, frame, edge=None):
        self.pts = np.asarray(block, dtype=F).reshape(-1, 3)
        self.e0 = edge0(max_dist) if edge is None else float(edge)
        self.nb = buckets_of(frame)
        lo = self.pts.min(axis=0).astype(np.float64)
        self.side = float((self.pts.max(axis=0).astype(np.float64) - lo).max())
        self.corner = lo
        self.e = max(self.e0, self.side * 2.0 ** -20)
        self.inv = 1.0 / self.e

    def cell(self, p):
        with np.errstate(invalid="ignore"):
            c = (np.asarray(p, dtype=F).astype(np.float64) - self.corner) * self.inv
        return tuple(int(v) for v in np.floor(np.clip(c, -1073741824.0, 1073741824.0)))

    def bucket(self, cell):
        return int(ol_hash(*cell)) & (self.nb - 1)

    def walk(self, cell):
        """The 27 cells around `cell` in the kernel's order (the own cell first) and their buckets."""
        cells = [(cell[0] + q % 3 - 1, cell[1] + (q // 3) % 3 - 1, cell[2] + q // 9 - 1) for q in WALK]
        return cells, [self.bucket(c) for c in cells]

    def count(self, i, thr, dedupe=True, test=True):
        """The neighbours vertex i's walk finds: every bucket once (dedupe) or once per cell that hashes to it, every candidate held
        to d^2 <= thr (test) or counted as it comes."""
        keys = [self.bucket(self.cell(p)) for p in self.pts]
        _, bk = self.walk(self.cell(self.pts[i]))
        if dedupe:
            bk = list(dict.fromkeys(bk))
        d = ref.dist2(self.pts[i:i + 1], self.pts)[0]
        return sum(int(sum(1 for j, kj in enumerate(keys) if kj == b and (not test or d[j] <= thr))) for b in bk)


WALK = [13] + list(range(13)) + list(range(14, 27))


def ol_hash(cx, cy, cz):
    m = 0xFFFFFFFF
    h = ((cx & m) * 73856093 & m) ^ ((cy & m) * 19349663 & m) ^ ((cz & m) * 83492791 & m)
    h ^= h >> 16
    h = h * 0x85EBCA6B & m
    h ^= h >> 13
    return h


def up(x, steps=1):
    x = F(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F(np.inf) if steps > 0 else F(-np.inf))
    return x


def d2(p, q):
    return ref.dist2(np.asarray(q, F).reshape(1, 3), np.asarray(p, F).reshape(1, 3))[0, 0]


def exact_root(v):
    """A float m with fl(m * m) == v, or None."""
    m = F(np.sqrt(np.float64(v)))
    for c in (m, up(m, -1), up(m, 1), up(m, -2), up(m, 2)):
        if F(c * c) == v and v > 0:
            return F(c)
    return None


def only(case):
    assert len(case.ticks) == 1 and len(case.ticks[0]) == 1
    return case.ticks[0][0], case.keep()[0][0]


CASES = []


def add(*a, **kw):
    CASES.append(Case(*a, **kw))


# ---- threshold on a pair ---------------------------------------------------------------------------------------------------------
# p = 0, q = a direction's vector: d = q - 0 is exact.  "diff": an anchor 0.9 e below p on every axis is the box's corner, so q lies in
# the next cell along every axis of the direction; "same": p is the corner and q shares its cell.  The anchor is further than maxDist
# from both.  at / below / above: d^2 == thr, one float step below, one above (on an axis, where no float's square lies one step from
# 2^-14, d is 2^-7 and its two neighbours: d^2 ==, <, > thr); k = 2, so q alone decides p.
M7 = F(2.0 ** -7)
THR7 = F(2.0 ** -14)
DIRECTIONS = {"x": (1, 0, 0), "y": (0, 1, 0), "z": (0, 0, 1), "xy": (1, 1, 0), "xz": (1, 0, 1), "yz": (0, 1, 1), "xyz": (1, 1, 1),
              "xYz": (1, -1, 1)}


@functools.lru_cache(maxsize=None)
def diagonal_pairs(name):
    """For a diagonal: (maxDist m, {step: q}) with thr = fl(m * m) the at-pair's own d^2 and the two others one float step off it.
    A seeded search: components near |q| = 2^-7 / sqrt(axes), moved by a few float steps."""
    axes = DIRECTIONS[name]
    rng = np.random.default_rng([20261021, sum(ord(c) for c in name)])
    n_axes = sum(1 for a in axes if a)
    for _ in range(2000):
        base = [F(a * rng.uniform(0.85, 1.15) * 2.0 ** -7 / np.sqrt(n_axes)) for a in axes]
        v = d2((0, 0, 0), base)
        m = exact_root(v)
        if m is None:
            continue
        found = {"at": np.array(base, F)}
        nz = [i for i, a in enumerate(axes) if a]
        for steps in itertools.product(range(-6, 7), repeat=len(nz)):
            q = list(base)
            for i, s in zip(nz, steps):
                q[i] = up(q[i], s * (1 if q[i] > 0 else -1))
            w = d2((0, 0, 0), q)
            if w == up(v, -1):
                found.setdefault("below", np.array(q, F))
            if w == up(v, 1):
                found.setdefault("above", np.array(q, F))
        if len(found) == 3:
            return m, found
    raise AssertionError(name)


def pair_case(direction, where, step):
    axes = DIRECTIONS[direction]
    on_axis = sum(1 for a in axes if a) == 1
    if on_axis:   # d one float step either side of 2^-7 (the square of a float cannot lie one step from 2^-14)
        m = M7
        q = np.array(axes, F) * {"at": M7, "below": up(M7, -1), "above": up(M7, 1)}[step]
    else:
        m, qs = diagonal_pairs(direction)
        q = qs[step]
    thr = ref.threshold(m)
    e = edge0(m)
    pts = [np.zeros(3, F), q]
    if where == "diff":
        pts.append([F(-0.9 * e) if a >= 0 else F(q[i] - F(0.9 * e)) for i, a in enumerate(axes)])
    block = np.array(pts, F)

    def witness(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        delta = tuple(x - y for x, y in zip(g.cell(b[1]), g.cell(b[0])))
        dd = d2(b[0], b[1])
        if on_axis:
            assert thr == THR7 and np.abs(b[1]).max() == {"at": M7, "below": up(M7, -1), "above": up(M7, 1)}[step]
            assert (dd == thr, dd < thr, dd > thr) == (step == "at", step == "below", step == "above"), (c.name, dd, thr)
        else:
            assert dd == {"at": thr, "below": up(thr, -1), "above": up(thr, 1)}[step], (c.name, dd, thr)
        assert delta == ((0, 0, 0) if where == "same" else axes), (c.name, delta)
        assert keep[0] == keep[1] == (step != "above"), (c.name, keep)
        assert len(b) == 2 or not keep[2]
    return Case(f"pair_{direction}_{where}_{step}", [FRAME_4096], [[block]], 2, m, witness)


for _d, _w, _s in itertools.product(DIRECTIONS, ("same", "diff"), ("at", "below", "above")):
    CASES.append(pair_case(_d, _w, _s))


# ---- all 26 neighbour cells ------------------------------------------------------------------------------------------------------
# An anchor at the corner, p in the middle of a cell, one satellite 0.55 e along the direction: in the neighbour cell, within maxDist.
# k = 2: the satellite alone decides p.  The cell of p is searched so that the satellite's cell has a bucket no other of the 27 has.
def neighbour_case(index, delta):
    m = F(0.01)
    e = edge0(m)
    frame = (FRAME_64, FRAME_PAST)[index % 2]
    for base in itertools.product(range(1, 7), repeat=3):
        p = np.array([(b + 0.5) * e for b in base], F)
        block = np.array([np.zeros(3, F), p, p + np.array(delta, F) * F(0.55 * e)], F)
        g = Grid(block, m, frame)
        cells, bk = g.walk(g.cell(block[1]))
        cs = g.cell(block[2])
        if cs in cells and bk.count(g.bucket(cs)) == 1:
            break
    else:
        raise AssertionError(delta)

    def witness(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        assert tuple(x - y for x, y in zip(g.cell(b[2]), g.cell(b[1]))) == tuple(delta), c.name
        assert g.walk(g.cell(b[1]))[1].count(g.bucket(g.cell(b[2]))) == 1
        assert d2(b[1], b[2]) <= ref.threshold(c.max_dist)
        assert keep.tolist() == [False, True, True], (c.name, keep)
        assert ref.keep_mask(b[:2], c.k, c.max_dist).tolist() == [False, False]      # without the satellite p is removed
    tag = "".join("mzp"[d + 1] for d in delta)
    return Case(f"cell_{tag}", [frame], [[block]], 2, m, witness)


NEIGHBOURS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
for _i, _delta in enumerate(NEIGHBOURS):
    CASES.append(neighbour_case(_i, _delta))


# ---- a shared bucket that decides ------------------------------------------------------------------------------------------------
# 64 buckets.  A seeded search over positions for a vertex whose own cell shares its bucket with another of its 27 cells.
@functools.lru_cache(maxsize=None)
def shared_positions():
    """(p whose own bucket is another walked cell's too, p whose own bucket is that of a far cell, that far cell's centre)."""
    m = F(0.01)
    e = edge0(m)
    rng = np.random.default_rng(20261022)
    near = far = None
    tried = 0
    while near is None or far is None:
        tried += 1
        assert tried < 1000
        p = (rng.uniform(2.0, 12.0, 3) * e).astype(F)
        g = Grid(np.array([np.zeros(3, F), p, np.full(3, F(16 * e))], F), m, FRAME_64)
        cell = g.cell(p)
        cells, bk = g.walk(cell)
        if near is None and bk[0] in bk[1:]:
            near = p
        if far is None and bk.count(bk[0]) == 1:
            for fc in itertools.product(range(0, 15), repeat=3):
                if max(abs(a - b) for a, b in zip(fc, cell)) >= 3 and g.bucket(fc) == bk[0]:
                    far = (p, np.array([(c + 0.5) * e for c in fc], F))
                    break
    return near, far[0], far[1], tried


def _shared_cases():
    m = F(0.01)
    thr = ref.threshold(m)
    e = edge0(m)
    near, p_far, far_centre, _ = shared_positions()
    top = np.full(3, F(16 * e))     # with the anchor at 0: the box the search assumed

    def lone(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        bk = g.walk(g.cell(b[1]))[1]
        assert g.nb == 64 and bk[0] in bk[1:]
        assert g.count(1, thr) == 1 < c.k <= g.count(1, thr, dedupe=False), c.name       # walked twice, it would be kept
        assert not keep[1]
    add("shared_lone", [FRAME_64], [[np.array([np.zeros(3, F), near, top], F)]], 2, m, lone)

    def k_minus_1(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        assert g.cell(b[1]) == g.cell(b[3]) and g.walk(g.cell(b[1]))[1][0] in g.walk(g.cell(b[1]))[1][1:]
        for i in (1, 3):
            assert g.count(i, thr) == c.k - 1 and g.count(i, thr, dedupe=False) >= c.k and not keep[i], c.name
    add("shared_k_minus_1", [FRAME_64], [[np.array([np.zeros(3, F), near, top, near + F(1e-4)], F)]], 3, m, k_minus_1)

    def far(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        cp, cf = g.cell(b[1]), g.cell(b[3])
        assert g.cell(b[4]) == cf == g.cell(b[5]) and max(abs(x - y) for x, y in zip(cp, cf)) >= 3
        assert g.bucket(cp) == g.bucket(cf) and g.walk(cp)[1].count(g.bucket(cp)) == 1
        assert g.count(1, thr) == 1 < c.k <= g.count(1, thr, test=False), c.name          # tested, not counted
        assert keep.tolist() == [False, False, False, True, True, True]
    cluster = [far_centre, far_centre + F(1e-4), far_centre - F(1e-4)]
    add("shared_far", [FRAME_64], [[np.array([np.zeros(3, F), p_far, top] + cluster, F)]], 2, m, far)


_shared_cases()


# ---- the self and duplicates -----------------------------------------------------------------------------------------------------
def _scatter(n, seed, spread=1.0, offset=0.0):
    """n points no two of which are within 0.05 * spread: a jittered lattice."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    lat = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n]
    return ((lat * 0.1 + rng.uniform(-0.02, 0.02, (n, 3))) * spread + offset).astype(F)


def _self_cases():
    cloud = _scatter(40, 1) - F(0.2)
    for tag, m in (("1e-30", 1e-30), ("1e-20", 1e-20), ("5cm", 0.05)):
        def k1(c, tag=tag):
            b, keep = only(c)
            assert keep.all() and not c.keep(rules=["self_not_counted"])[0][0].any(), c.name
            assert (ref.threshold(c.max_dist) == 0) == (tag == "1e-30")
        add(f"k1_{tag}", [FRAME_64], [[cloud]], 1, m, k1)
    P = np.array([0.25, -0.5, 1.0], F)
    others = np.array([[0, 0, 0], [1, 1, 1], [-1, 0.5, 2]], F)
    for tag, m in (("sq0", 1e-30), ("sqsub", 1e-20)):
        for k in (5, 6):
            def dup(c, k=k, tag=tag):
                b, keep = only(c)
                thr = ref.threshold(c.max_dist)
                assert thr == 0 if tag == "sq0" else 0 < thr < np.finfo(F).tiny
                assert (b[1:6] == P).all() and keep[1:6].tolist() == [k == 5] * 5 and not keep[0] and not keep[6:].any(), c.name
            add(f"dup5_k{k}_{tag}", [FRAME_64], [[np.concatenate([others[:1], np.tile(P, (5, 1)), others[1:]])]], k, m, dup)
    # key runs of ol_runs: 64 identical points fill a wave, 65 cross into the next, 129 cross a workgroup of 256 lanes and end on a
    # wave's first lane
    runs = {"run64": (0, 64, 1, FRAME_PAST, 1e-30), "run65": (5, 65, 2, (9, 8), 0.01), "run129": (192, 129, 3, (18, 18), 0.01)}
    for tag, (before, j, after, frame, m) in runs.items():
        block = np.concatenate([_scatter(before, 2, offset=2.0), np.tile(P, (j, 1)), _scatter(after, 3, offset=-3.0)])
        for k in (j, j + 1):
            def run(c, k=k, j=j, before=before):
                b, keep = only(c)
                assert (b[before:before + j] == P).all() and len(np.unique(b, axis=0)) == len(b) - j + 1
                first, last = before, before + j - 1
                assert {"run64": first % 64 == 0 and last % 64 == 63, "run65": first // 64 + 1 == last // 64,
                        "run129": first // 256 + 1 == last // 256 and last % 64 == 0}[c.name.split("_")[0]]
                assert keep[first:last + 1].tolist() == [k == j] * j and keep.sum() == (j if k == j else 0), c.name
            add(f"{tag}_k{k}", [frame], [[block]], k, m, run)


_self_cases()


# ---- small blocks ----------------------------------------------------------------------------------------------------------------
def largest_finite_root():
    """The float m whose float square is the largest finite float square."""
    m = F(np.sqrt(np.float64(np.finfo(F).max)))
    with np.errstate(over="ignore"):
        while np.isinf(m * m):
            m = up(m, -1)
        while not np.isinf(up(m, 1) * up(m, 1)):
            m = up(m, 1)
    return m


def _small_cases():
    k = 4
    rng = np.random.default_rng(4)
    tight = [(c + rng.uniform(-0.001, 0.001, (n, 3))).astype(F) for n, c in ((k - 1, -1.0), (0, 0.0), (k, 0.5), (k + 1, 2.0))]
    wide = [(b * F(1000)).astype(F) for b in tight]
    settings = {"finite": (tight, 0.05), "spread": (wide, 0.05), "largest": (wide, largest_finite_root()), "inf": (wide, 1e30),
                "maxdist_inf": (wide, np.inf)}
    for tag, (blocks, m) in settings.items():
        def small(c, tag=tag):
            thr = ref.threshold(c.max_dist)
            keep = c.keep()[0]
            assert [len(b) for b in c.ticks[0]] == [k - 1, 0, k, k + 1] and c.k == k
            assert {"finite": np.isfinite(thr), "spread": np.isfinite(thr), "largest": np.isfinite(thr) and thr > F(3.4e38),
                    "inf": np.isinf(thr), "maxdist_inf": np.isinf(c.max_dist)}[tag]
            assert keep[0].tolist() == [bool(np.isinf(thr))] * (k - 1), c.name          # FLT_MAX > thr unless thr is inf
            assert keep[2].tolist() == [tag != "spread"] * k and keep[3].tolist() == [tag != "spread"] * (k + 1), c.name
            assert c.counts()[0][1] == [0, 0, k, k + 1]
        add(f"small_{tag}", [FRAME_64] * 4, [blocks], k, m, small)


_small_cases()


# ---- sensor and tick scoping -----------------------------------------------------------------------------------------------------
def _mix(n, lone, seed):
    """n points in one region whatever the seed: n - lone on a line 2 mm apart (each within 5 mm of two others), `lone` points 1 m
    apart at places that do not depend on the seed (so the same lone points appear in every block), half in front, half behind."""
    rng = np.random.default_rng(seed)
    dense = n - lone
    line = np.stack([np.arange(dense) * 0.002, np.full(dense, rng.uniform(0, 0.001)), np.zeros(dense)], 1)
    lonely = np.stack([5.0 + np.arange(lone), np.full(lone, -3.0), np.full(lone, 2.0)], 1)
    return np.concatenate([lonely[:lone // 2], line, lonely[lone // 2:]]).astype(F)


def _scope_cases():
    m = F(0.01)
    pairs = np.concatenate([[[i * 0.5, -0.25, 0.1], [i * 0.5 + 0.004, -0.25, 0.1]] for i in range(6)]).astype(F)

    def sensors(c):
        assert all(not keep.any() for keep in c.keep()[0]) and all(keep.all() for keep in c.keep(rules=["scope_tick"])[0]), c.name
        assert (ref.neighbour_counts(pairs, ref.threshold(m)) == c.k - 1).all()
    add("scope_sensors", [FRAME_64] * 2, [[pairs, pairs]], 3, m, sensors)

    def ticks(c):
        assert all(not row[0].any() for row in c.keep()) and all(not row[0].any() for row in c.keep(rules=["scope_tick"])), c.name
        assert all(row[0].all() for row in c.keep(rules=["scope_batch"]))
    add("scope_ticks", [FRAME_64], [[pairs], [pairs]], 3, m, ticks)

    for tag, sizes, lone in (("a", (1, 63, 64, 65, 100, 1), (1, 3, 10, 0, 37, 1)), ("b", (63, 1, 64, 65, 100, 1), (3, 1, 10, 0, 37, 1))):
        frames = [(10, 10) if n == 100 else (65, 1) if n == 65 else FRAME_64 for n in sizes]

        def bounds(c, sizes=sizes, lone=lone):
            removed, exact = c.counts()[0]
            assert removed == list(lone) and exact == [n if n >= c.k else 0 for n in sizes], (c.name, removed, exact)
            assert all(removed[i] != removed[i + 1] and exact[i] != exact[i + 1] for i in range(len(sizes) - 1))
            lanes = [int(o) % 64 for o in np.cumsum(sizes)[:-1]]
            assert lanes == ([1, 0, 0, 1, 37] if sizes[0] == 1 else [63, 0, 0, 1, 37])
            wrong = c.keep(rules=["scope_tick"])[0]       # the same lone points lie in the neighbouring blocks
            assert sum(int((~w).sum()) for w in wrong) < sum(removed)
        add(f"boundaries_{tag}", frames, [[_mix(n, r, 10 + i) for i, (n, r) in enumerate(zip(sizes, lone))]], 2, F(0.005), bounds)

    sizes3 = [[(5, 2), (0, 0), (20, 3)], [(0, 0), (33, 4), (7, 7)], [(64, 1), (64, 0), (1, 1)]]

    def three(c):
        offs = [np.cumsum([0] + [len(b) for b in tick]).tolist() for tick in c.ticks]
        assert len({tuple(o) for o in offs}) == 3
        assert [r for r, _ in c.counts()] == [[2, 0, 3], [0, 4, 7], [1, 0, 1]], c.counts()
        assert [e for _, e in c.counts()] == [[5, 0, 20], [0, 33, 7], [64, 64, 0]]
    add("ticks3", [FRAME_64] * 3, [[_mix(n, r, 30 + 3 * t + s) for s, (n, r) in enumerate(row)] for t, row in enumerate(sizes3)], 2, F(0.005),
        three)


_scope_cases()


# ---- box and sign ----------------------------------------------------------------------------------------------------------------
def _box_cases():
    sub = F(1e-40)
    tiny = F(1.4e-45)
    zeros = np.array([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [sub, -sub, 0.0], [-sub, 0.0, sub], [tiny, 0.0, -0.0], [-tiny, F(1e-39), 0.0]], F)
    far = np.array([[1, 0.5, -1], [-1, -0.5, 1], [0.5, -1, 0.25], [-0.25, 1, -0.5], [1e-3, -1e-3, 1e-3], [-1e-3, 1e-3, -1e-3]], F)
    block = np.concatenate([far[:3], zeros, far[3:]])
    for tag, k, m in (("k6_sq0", 6, 1e-30), ("k7_sq0", 7, 1e-30), ("k6_sqsub", 6, 1e-20), ("k2_1mm", 2, 1e-3)):
        def sign(c, tag=tag):
            b, keep = only(c)
            z = b[3:9]
            assert np.signbit(z[1]).all() and not np.signbit(z[0]).any() and (z[0] == z[1]).all()        # -0.0 and +0.0, both there
            assert ((np.abs(z) > 0) & (np.abs(z) < np.finfo(F).tiny)).sum() >= 6 and (b.min(0) < 0).all() and (b.max(0) > 0).all()
            assert (ref.dist2(z, z) == 0).all()               # d^2 of subnormal differences underflows
            assert keep[3:9].tolist() == [tag != "k7_sq0"] * 6 and not keep[:3].any() and not keep[9:].any(), (c.name, keep)
        add(f"sign_{tag}", [FRAME_64], [[block]], k, m, sign)

    lat = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cloud = np.concatenate([(lat - 3.5) * 0.0007, [[4000.0, 0.0, 0.0]]]).astype(F)

    def huge(c):
        b, keep = only(c)
        g = Grid(b, c.max_dist, c.frames[0])
        assert g.e > g.e0 and g.e == g.side * 2.0 ** -20 and g.e > 3 * float(c.max_dist)
        assert 0 < keep.sum() < len(b) - 1 and not keep[-1], (c.name, int(keep.sum()))
        assert len({g.cell(p) for p in b[:-1]}) >= 2         # the lattice still spans a cell border
    add("box_4000m", [(23, 23)], [[cloud]], 14, 1e-3, huge)

    same = np.tile(np.array([0.3, -0.2, 1.5], F), (10, 1))
    for k in (10, 11):
        def coincide(c, k=k):
            b, keep = only(c)
            g = Grid(b, c.max_dist, c.frames[0])
            assert g.side == 0 and g.e == g.e0 and keep.tolist() == [k == 10] * 10
        add(f"coincide_k{k}", [FRAME_POW2], [[same]], k, 0.01, coincide)

    for tag, frame, n in (("64", FRAME_64, 60), ("pow2", FRAME_POW2, 64), ("past", FRAME_PAST, 65)):
        rng = np.random.default_rng(n)
        pts = np.concatenate([rng.normal(0, 0.03, (n - 10, 3)), rng.uniform(-1, 1, (10, 3))]).astype(F)

        def table(c, frame=frame):
            b, keep = only(c)
            assert buckets_of(frame) == {FRAME_64: 64, FRAME_POW2: 64, FRAME_PAST: 128}[frame] and 0 < keep.sum() < len(b)
        add(f"random_{tag}", [frame], [[pts]], 3, 0.02, table)


_box_cases()


# ---- arithmetic: pairs that tell the roundings apart ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def arithmetic_pair(rule):
    """A seeded search for (p, q, maxDist): thr = fl(maxDist^2) is the pair's own d^2, and `rule` puts the pair beyond its threshold."""
    rng = np.random.default_rng([20261023, sorted(ref.RULES).index(rule)])
    for tried in range(1, 20001):
        p = rng.uniform(-1, 1, 3).astype(F)
        q = (p + rng.normal(0, 0.01, 3)).astype(F)
        v = d2(p, q)
        m = exact_root(v)
        if m is None:
            continue
        if rule == "thr_double":
            if np.float64(m) ** 2 < np.float64(v):
                return p, q, m, tried
        elif ref._wrong_dist2(q[None], p[None], {rule})[0, 0] > v:
            return p, q, m, tried
    raise AssertionError(rule)


for _rule in ("thr_double", "d2_double", "d2_right_to_left", "d2_fma"):
    def _arith(c, rule=_rule):
        b, keep = only(c)
        assert d2(b[0], b[1]) == ref.threshold(c.max_dist) and keep.all() and not c.keep(rules=[rule])[0][0].any(), c.name
    _p, _q, _m, _ = arithmetic_pair(_rule)
    add(f"arith_{_rule}", [FRAME_64], [[np.array([_p, _q], F)]], 2, _m, _arith)


# ---- a candidate for the edge's slack --------------------------------------------------------------------------------------------
EDGE_BUDGET = 400_000
EDGE_SEED = 20261024


@functools.lru_cache(maxsize=None)
def edge_slack_search(budget=EDGE_BUDGET, seed=EDGE_SEED):
    """A pair on the x axis with |q - p| > maxDist in the reals and fl(fl(q - p)^2) <= thr, whose cells lie two apart when the edge is
    maxDist itself and one apart with the kernel's edge; the box's corner is an anchor's x.  Candidates: p in (-maxDist / 2,
    -maxDist / 8), q the float sum maxDist + p moved up by 0 .. 2 float steps (the difference then rounds), the anchor 2 or 3 edges
    below, at the float nearest to where a cell border falls between p and q - maxDist.  Returns (block, maxDist, hits, budget) or None."""
    rng = np.random.default_rng(seed)
    m = rng.uniform(1e-3, 1e-1, budget).astype(F)
    p = (-m * rng.uniform(0.125, 0.5, budget).astype(F)).astype(F)
    q = (m + p).astype(F)
    steps = rng.integers(0, 3, budget)
    for s in (1, 2):
        q = np.where(steps >= s, np.nextafter(q, F(np.inf)), q).astype(F)
    j = rng.integers(2, 4, budget)
    m64, p64, q64 = m.astype(np.float64), p.astype(np.float64), q.astype(np.float64)
    real = q64 - p64                                  # exact: both are floats of nearby exponents
    c = (p64 + (real - m64) / 2 - j * m64).astype(F)
    c64 = c.astype(np.float64)
    dfl = (q - p).astype(F)
    ok = (real > m64) & ((dfl * dfl).astype(F) <= (m * m).astype(F)) & (c < p)

    def cells(edge):
        inv = 1.0 / edge
        return np.floor((p64 - c64) * inv), np.floor((q64 - c64) * inv)
    a0, b0 = cells(m64)
    a1, b1 = cells(m64 * (1.0 + 2.0 ** -20) + 2.0 ** -70)
    ok &= (b0 - a0 == 2) & (b1 - a1 == 1)
    hits = np.flatnonzero(ok)
    if len(hits) == 0:
        return None
    i = int(hits[0])
    block = np.array([[c[i], 0.5, 0.0], [p[i], 0.0, 0.0], [q[i], 0.0, 0.0]], F)
    return block, m[i], len(hits), budget


def _edge_case():
    found = edge_slack_search()
    if found is None:
        return
    block, m, _, _ = found

    def slack(c):
        b, keep = only(c)
        md = float(c.max_dist)
        assert float(b[2, 0]) - float(b[1, 0]) > md and d2(b[1], b[2]) <= ref.threshold(c.max_dist)
        for edge in (md, md + 2.0 ** -70):            # the edge without its slack: the pair's cells are not neighbours
            g = Grid(b, c.max_dist, c.frames[0], edge=edge)
            assert g.e == edge and g.cell(b[2])[0] - g.cell(b[1])[0] == 2
        g = Grid(b, c.max_dist, c.frames[0])
        assert g.e == g.e0 and g.cell(b[2])[0] - g.cell(b[1])[0] == 1
        assert keep.tolist() == [False, True, True]
    add("edge_slack", [FRAME_64], [[block]], 2, m, slack)


_edge_case()

NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

