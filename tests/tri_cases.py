"""Inputs that put the triangulation on its decision boundaries: depth windows built FROM the threshold, laid out in frames.
TEST INFRASTRUCTURE ONLY: pure functions, no torch, no native library; shared by tests/test_tri_boundary_ref.py (CPU),
tests/test_tri_boundary_gpu.py and tests/golden/make_tri_golden.py.

A pixel P = (x, y) with the corners U = (x, y-1), UR = (x+1, y-1), R = (x+1, y) reads a 4 x 4 window, rows y-2 .. y+1 and columns
x-1 .. x+2: the four corners and the 12 probes of the six edge directions, 16 distinct positions, no probe a corner.  A STENCIL is one
such window W[dy + 2][dx + 1] built for a target (level, triangle, edge, rule, margin): the one difference that decides the triangle sits
on thr - 1 (accept) or on thr (reject), every other rule of that edge fails, the triangle's other edges pass.  build_stencil() verifies
that with the instrumented restatement (tests/tri_ref.py) before it returns a window, so a frame holds only windows that are what they
are labelled."""
import functools

import numpy as np

from tests import tri_ref
from tests.tri_ref import CHECK_CORNERS, RULES

LEVELS = (120, 1500, 30000, 62000)
MARGINS = ("accept", "reject")
CUT = 65000                                                      # the deepest depth with a vertex under BOX (65.0 is not > 65.0)
BOX = np.array([-100, -100, -100, 100, 100, 65.0], dtype=np.float32)      # the frames' crop box: wide in X / Y, maxZ on the cut
WIDE_BOX = np.array([-100, -100, -100, 100, 100, 100], dtype=np.float32)   # ... and one under which every depth has a vertex
POSE = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float32)    # identity: t, then R row-major
TILE = 2048                                                      # pixels per tile of the triangle passes (fusion_shared.hpp: kTile)
UR_PROBES = ((2, 1), (-1, -2))                                   # the probes of edge U - R, which only triangles 0 and 1 use


def intrinsics(w, h):
    """A pinhole whose rays stay inside BOX's X / Y at every depth a u16 holds, for every frame here."""
    return np.array([(w - 1) / 2.0, (h - 1) / 2.0, 365.0, 365.0, 0, 0, 0], dtype=np.float32)


def all_targets():
    """(triangle, edge, rule, margin): 4 x 3 x 3 x 2 = 72."""
    return [(i, j, r, m) for i in range(4) for j in range(3) for r in RULES for m in MARGINS]


def _cell(W, d):
    return W[d[1] + 2][d[0] + 1]


def _set(W, d, v):
    W[d[1] + 2][d[0] + 1] = v


def _window(L, thr, i, j, rule, margin, sign, other_off, sa, sb, nudge=(0, 0)):
    """One attempt at the target with the threshold ASSUMED to be thr; the caller recomputes it from the corners."""
    T = thr + 2
    a, b = sa * (2 * T + 3), sb * (5 * T + 1)         # |a|, |b|, |a +- b| >= thr + 2: every edge fails the absolute rule, passes the forward one with 0
    m = thr - 1 if margin == "accept" else thr
    c = CHECK_CORNERS[i]
    A, B = c[j], c[(j + 1) % 3]
    ex, ey = B[0] - A[0], B[1] - A[1]
    if rule == "abs":                                  # a ex + b ey = sign m
        if ey == 0:
            a = sign * m * ex
        elif ex == 0:
            b = sign * m * ey
        else:
            b = ey * (sign * m - a * ex)
    W = [[L + a * dx + b * dy for dx in range(-1, 3)] for dy in range(-2, 2)]
    for d, v in ((A, nudge[0]), (B, nudge[0]), (c[(j + 2) % 3], nudge[1])):     # moves the corner sum; the target edge keeps its difference
        _set(W, d, _cell(W, d) + v)
    fpos, bpos = (B[0] + ex, B[1] + ey), (A[0] - ex, A[1] - ey)
    va, vb = _cell(W, A), _cell(W, B)
    push = thr + 5
    zeroed = set()

    def probe(d, v):
        _set(W, d, v)
        if v == 0:
            zeroed.add(d)

    if rule == "abs":                                  # both probes 0: this compare alone decides
        probe(fpos, 0)
        probe(bpos, 0)
    elif rule == "fwd":
        probe(fpos, 2 * vb - va + sign * m)
        probe(bpos, 2 * va - vb + sign * push if other_off else 0)
    else:
        probe(bpos, 2 * va - vb + sign * m)
        probe(fpos, 2 * vb - va + sign * push if other_off else 0)
    if i >= 2:                                         # 2 and 3 are evaluated only when 0 and 1 fail: their shared edge U - R then must
        for d in UR_PROBES:
            probe(d, 0)
    if any(not 1 <= _cell(W, (dx, dy)) <= CUT for dx in range(-1, 3) for dy in range(-2, 2) if (dx, dy) not in zeroed):
        return None
    return W


def _verify(W, i, j, rule, margin):
    """Is W what its label says?  Judged by the instrumented restatement alone."""
    d = np.array(W, dtype=np.int64)
    t = tri_ref.trace_triangle(d, 1, 2, i)
    if t is None:
        return False
    thr, e = t["thr"], t["edges"][j]
    if e[rule] != (thr - 1 if margin == "accept" else thr):
        return False
    if any(e[r] is not None and e[r] < thr for r in RULES if r != rule):
        return False
    if any(not any(o[r] is not None and o[r] < thr for r in RULES) for k, o in enumerate(t["edges"]) if k != j):
        return False
    if t["verdict"] != (margin == "accept"):
        return False
    if i >= 2:
        for k in (0, 1):
            tk = tri_ref.trace_triangle(d, 1, 2, k)
            if tk is not None and tk["verdict"]:
                return False
    return True


def build_stencil(L, i, j, rule, margin, sign=1, other_off=False, nudge=(0, 0), thr0=None):
    """The 4 x 4 window (list of rows, ints in [0, CUT]) for the target, P at depth L.  The threshold depends on the corners and the
    corners on the threshold: iterated until it no longer moves.  The ramp's direction is flipped when the window would leave the depth
    range.  nudge = (both ends of the target edge, the third corner): a few units added to the corners after the ramp, to steer their
    sum, and thr0 = where the threshold's iteration starts (exact_sum_stencils: where the threshold steps, two windows are consistent).
    Raises when the target cannot be reached."""
    for sa, sb in ((1, 1), (-1, 1), (1, -1), (-1, -1)):
        thr = tri_ref.threshold(L, L, L) if thr0 is None else thr0
        for _ in range(8):
            W = _window(L, thr, i, j, rule, margin, sign, other_off, sa, sb, nudge)
            if W is None:
                break
            actual = tri_ref.threshold(*[_cell(W, d) for d in CHECK_CORNERS[i]])
            if actual == thr:
                if _verify(W, i, j, rule, margin):
                    return W
                break
            thr = actual
    raise ValueError(f"unreachable target {(L, i, j, rule, margin, sign, other_off)}")


def _corner_sum(W, i):
    return sum(_cell(W, d) for d in CHECK_CORNERS[i])


@functools.lru_cache(maxsize=None)
def exact_sum_stencils():
    """Targets whose corner sum s puts the division-free compare ON equality: the kernel accepts 18750 m <= 17 s + 117618.  Accept
    margin: 17 s + 117618 is a multiple of 18750, so the metric thr - 1 gives 18750 m == 17 s + 117618 -- a constant one too small, or
    < for <=, rejects it.  Reject margin: 17 s + 117618 == -1 (mod 18750), so the metric thr gives 18750 m == 17 s + 117618 + 1 -- a
    constant one too large accepts it.  17 is invertible mod 18750: one sum in 18 750 qualifies, ten or so over the depth range; the
    level is solved for from the sum, triangle by triangle.  [(window, "exact", (level, triangle, edge, rule, margin), None)]: every
    triangle and margin with (edge 0, abs), (edge 1, fwd), (edge 2, bwd), walking through the qualifying sums."""
    out, n = [], 0
    for margin in MARGINS:
        res = 0 if margin == "accept" else 18749
        sums = [t for t in range(400, 3 * CUT - 3000) if (17 * t + 117618) % 18750 == res]
        for i in range(4):
            for j, rule in ((0, "abs"), (1, "fwd"), (2, "bwd")):
                found = None
                for k in range(len(sums)):
                    want = sums[(n + k) % len(sums)]
                    thr_want = tri_ref.threshold(want, 0, 0)
                    for variant in range(4):
                        sign, other_off = (1, -1)[variant % 2], bool(variant // 2)
                        try:
                            c = _corner_sum(build_stencil(want // 3, i, j, rule, margin, sign, other_off, thr0=thr_want), i) - 3 * (want // 3)
                        except ValueError:
                            continue
                        # s = 3 L + c, but c moves with the threshold and the threshold steps exactly at these sums: the corners
                        # themselves are nudged by a few units to land on the sum
                        tries = [(L, (n2, n1)) for L in range((want - c) // 3 - 2, (want - c) // 3 + 3) for n2 in (0, 1, -1) for n1 in (0, 1, -1, 2, -2)]
                        for L, nudge in tries:
                            try:
                                W = build_stencil(L, i, j, rule, margin, sign, other_off, nudge, thr_want)
                            except ValueError:
                                continue
                            if _corner_sum(W, i) == want:
                                found = (W, "exact", (_cell(W, (0, 0)), i, j, rule, margin), None)
                                break
                        if found:
                            break
                    if found:
                        break
                assert found, (i, j, rule, margin)
                out.append(found)
                n += 1
    return tuple(out)


def flat(v):
    return [[v] * 4 for _ in range(4)]


def _with(W, cells):
    W = [row[:] for row in W]
    for d, v in cells.items():
        _set(W, d, v)
    return W


_CORNERS = {"P": (0, 0), "U": (0, -1), "UR": (1, -1), "R": (1, 0)}
_PROBES = [(dx, dy) for dx in range(-1, 3) for dy in range(-2, 2) if (dx, dy) not in _CORNERS.values()]


def special_stencils():
    """The hand-made windows and the ones with depth but no vertex: [(name, window, expected)].  `expected`: None = whatever the
    reference says (the builder does not know), else the triangle numbers pixel P emits under BOX -- written out by hand."""
    far = CUT
    out = [
        # hand-made
        ("flat_65535", flat(65535), []),                               # under BOX no corner has a vertex; under WIDE_BOX: [0, 1]
        ("flat_1", flat(1), [0, 1]),
        ("mix_1_65535", _with(flat(1), {(1, 0): 65535, (0, -2): 65535, (2, -1): 0}), None),
        ("mix_65535_1_holes", _with(flat(65535), {(0, -1): 1, (-1, 0): 0, (2, 0): 0, (0, 1): 1}), None),
        ("mix_checker", [[1 if (r + c) % 2 else 65000 for c in range(4)] for r in range(4)], None),
        ("mix_holes_far", _with(flat(far), {(-1, -2): 0, (2, 1): 0, (1, -2): 1, (-1, 0): 65535}), None),
        ("probes_zero", _with(flat(0), {d: 1500 for d in _CORNERS.values()}), [0, 1]),
        ("probes_zero_steep", _with(flat(0), {(0, 0): 1500, (0, -1): 1500, (1, -1): 1600, (1, 0): 1500}), [0]),
    ]
    for name, d in _CORNERS.items():                                   # every corner zero in turn (P = 0: no vertex)
        want = {"P": [], "U": [3], "UR": [0], "R": [2]}[name]
        out.append((f"zero_{name}", _with(flat(1500), {d: 0}), want))
    # depth but no vertex (BOX: depths above CUT)
    out += [
        ("novertex_R", _with(flat(far), {_CORNERS["R"]: far + 100}), []),        # verdicts 0 and 1 true, nothing emitted -- NOT triangle 2
        ("novertex_U", _with(flat(far), {_CORNERS["U"]: far + 100}), []),        # 0 and 1 true and dropped; 3 never evaluated
        ("novertex_UR", _with(flat(far), {_CORNERS["UR"]: far + 100}), [0]),     # 0 emitted, 1 dropped
        ("novertex_P", _with(flat(far), {_CORNERS["P"]: far + 100}), []),        # P without a vertex is skipped
        ("novertex_R_max", _with(flat(far), {_CORNERS["R"]: 65535}), None),
        ("novertex_probes", _with(flat(far), {d: far + 1 for d in _PROBES}), [0, 1]),   # a probe above the cut is still a valid probe
    ]
    # ... a probe above the cut that DECIDES: U - R is steep and linear, only its forward probe (no vertex) lets triangle 0 and 1 pass
    W = flat(far - 600)
    for dx in range(-1, 3):
        for dy in range(-2, 2):
            _set(W, (dx, dy), far - 900 + 300 * (dx + dy))             # U = far - 1200, R = far - 600, forward probe (2, 1) = far
    _set(W, (2, 1), far + 1)                                           # |2 R - U - probe| = 1
    _set(W, (-1, -2), 0)
    out.append(("novertex_probe_decides", W, None))
    return out


class Frame:
    """depth (h, w) u16 and where its stencils lie: placements = [dict(x, y, kind, label, expected)], owner (h, w) int = the placement a
    pixel belongs to (-1: background)."""

    def __init__(self, name, w, h):
        self.name, self.w, self.h = name, w, h
        self.depth = np.zeros((h, w), dtype=np.uint16)
        self.owner = np.full((h, w), -1, dtype=np.int32)
        self.placements = []
        self.box = BOX

    def place(self, W, x, y, kind, label, expected=None):
        """The window with P at (x, y), clipped to the frame; no two windows may share a pixel."""
        k = len(self.placements)
        for r in range(4):
            for c in range(4):
                yy, xx = y - 2 + r, x - 1 + c
                if 0 <= yy < self.h and 0 <= xx < self.w:
                    assert self.owner[yy, xx] == -1, (self.name, label, x, y)
                    self.owner[yy, xx] = k
                    self.depth[yy, xx] = W[r][c]
        self.placements.append({"x": x, "y": y, "kind": kind, "label": label, "expected": expected})

    def with_background(self, kind, seed=20261018):
        """"holes": as built (every pixel outside a window is 0).  "dense": those pixels drawn over [1, CUT], no smoothness."""
        f = Frame(f"{self.name}_{kind}", self.w, self.h)
        f.owner, f.placements, f.box = self.owner, self.placements, self.box
        f.depth = self.depth.copy()
        if kind == "dense":
            rng = np.random.default_rng(seed)
            bg = rng.integers(1, CUT + 1, size=(self.h, self.w)).astype(np.uint16)
            f.depth = np.where(self.owner == -1, bg, self.depth).astype(np.uint16)
        else:
            assert kind == "holes"
        return f

    def describe(self, x, y):
        """Which stencil pixel (x, y) belongs to, for a failure message."""
        k = int(self.owner[y, x]) if 0 <= y < self.h and 0 <= x < self.w else -1
        if k < 0:
            return f"pixel ({x}, {y}) of {self.name}: background"
        p = self.placements[k]
        return f"pixel ({x}, {y}) of {self.name}: stencil {p['label']} ({p['kind']}) with P at ({p['x']}, {p['y']})"

    def rgb(self):
        yy, xx = np.mgrid[0:self.h, 0:self.w]
        return np.stack([xx * 3 % 256, yy * 5 % 256, (xx + yy) % 256], axis=-1).astype(np.uint8)


def _slots(w, col):
    return [8 * s + col for s in range(8) if 1 <= 8 * s + col <= w - 3]


def _lay_out(name, w, queues, lanes_block=False):
    """queues[col] = [(window, kind, label, expected)] to be laid at lane column col.  Bands of 4 rows, P at y = 4 band + 2, pitch 8; band k
    uses column k % 8.  Band 0 keeps its last slots free and one more band is added below for the windows that sit across the frame's
    limits.  lanes_block: a band of its own with a lane (columns 8 .. 15) whose pixels have depth but no vertex beside one (16 .. 23) that
    has some -- the VEC form skips the first lane's stencils, the second still reads it as `left` and through the compact map."""
    queues = [list(q) for q in queues]
    plan, band = [], 0
    while any(queues):
        col = band % 8
        xs = _slots(w, col)
        if band == 0:
            xs = [x for x in xs if x < 40]
        for x in xs:
            if queues[col]:
                plan.append((x, 4 * band + 2, queues[col].pop(0)))
        band += 1
    lanes_band = band if lanes_block else None
    last = band + (1 if lanes_block else 0)                 # one more band: P at y = h - 3, and beside it one at y = h - 2
    h = 4 * (last + 1) + 1
    f = Frame(name, w, h)
    for x, y, (W, kind, label, expected) in plan:
        f.place(W, x, y, kind, label, expected)
    if lanes_block:
        y0 = 4 * lanes_band
        f.depth[y0:y0 + 4, 8:16] = CUT + 7
        f.depth[y0:y0 + 4, 16:24] = CUT
        f.owner[y0:y0 + 4, 8:24] = len(f.placements)
        f.placements.append({"x": 15, "y": y0 + 2, "kind": "lanes", "label": "lane_without_vertices", "expected": []})
    edge = build_stencil(1500, 0, 0, "abs", "accept")       # emits triangle 0 wherever it lies inside the limits
    col = last % 8
    for x in _slots(w, col)[1:4]:
        f.place(edge, x, 4 * last + 2, "limit", "inside_y=h-3", None)
    f.place(edge, 48 + col % 4, 4 * last + 3, "limit", "across_y=h-2", [])
    f.place(edge, 48, 1, "limit", "across_y=1", [])
    f.place(edge, 0, 2, "limit", "across_x=0", [])
    k = (w - 2) % 8                                         # the first band of that lane column: its slot at x = w - 2 is free
    f.place(edge, w - 2, 4 * k + 2, "limit", "across_x=w-2", [])
    return f


def _entry(level, t, n):
    """The target's window in variant n: the sign of the margin and what the other probe is (0, or off by more than thr) alternate; a
    variant that leaves the depth range gives way to the next."""
    i, j, rule, margin = t
    for k in range(4):
        sign, other_off = (1, -1)[(n + k) % 2], bool(((n + k) // 2) % 2)
        try:
            return (build_stencil(level, i, j, rule, margin, sign, other_off), "target", (level, i, j, rule, margin), None)
        except ValueError:
            pass
    raise ValueError(f"unreachable target {(level,) + tuple(t)}")


def _specials():
    return [(W, "special", name, expected) for name, W, expected in special_stencils()]


def vec_frame():
    """Width 64 (the device-resident VEC form: 8 pixels per lane, widths % 8 == 0): every target and every special stencil at every lane
    column 0 .. 7; the level walks with the column, so every target meets every level.  The exact-sum stencils too lie at every column."""
    queues = [[] for _ in range(8)]
    for col in range(8):
        for n, t in enumerate(all_targets()):
            queues[col].append(_entry(LEVELS[(col + n // 2) % 4], t, n // 2 + col))   # accept and reject: same level, same variant
        queues[col] += list(exact_sum_stencils()) + _specials()
    return _lay_out("vec64", 64, queues, lanes_block=True)


def general_frame():
    """Width 61 (tiles begin mid-row, a lane's pixels span rows): every (level, target) once, every exact-sum and every special stencil once."""
    items = [_entry(L, t, n) for L in LEVELS for n, t in enumerate(all_targets())] + list(exact_sum_stencils()) + _specials()
    queues = [[] for _ in range(8)]
    for n, it in enumerate(items):
        queues[n % 8].append(it)
    return _lay_out("gen61", 61, queues)


def hand_frame(w):
    """The special stencils alone, under WIDE_BOX: there the windows at 65 535 have their vertices."""
    queues = [[] for _ in range(8)]
    for n, it in enumerate(_specials()):
        W, kind, label, expected = it
        queues[n % 8].append((W, kind, label, None))
    f = _lay_out(f"hand{w}", w, queues)
    f.box = WIDE_BOX
    return f


# ---- write-pass frames ------------------------------------------------------------------------------------------------------------

WRITE_DEPTH = 1500
WRITE_SIZES = ((64, 40), (61, 42))
WRITE_COUNTS = (0, 1, 15, 16, 17, 1535, 1536, 1537, 3071, 3072, 3073, "full")    # tile 0's triangles; 1536 = kTriWinDefault


def flat_counts(depth):
    """Triangles per pixel of a frame whose non-zero depths are all equal and all have vertices: every edge passes the absolute rule, a
    triangle exists iff its three corners do."""
    h, w = depth.shape
    v = depth != 0
    n = np.zeros((h, w), dtype=np.int64)
    Pm, Um, URm, Rm = v[2:h - 2, 1:w - 2], v[1:h - 3, 1:w - 2], v[1:h - 3, 2:w - 1], v[2:h - 2, 2:w - 1]
    t0, t1 = Pm & Um & Rm, Rm & Um & URm
    alt = ~(t0 | t1)
    t2, t3 = alt & Pm & Um & URm, alt & Pm & URm & Rm
    n[2:h - 2, 1:w - 2] = (t0 & Pm).astype(int) + (t1 & Pm) + t2 + t3
    return n


def tile_counts(depth):
    c = flat_counts(depth).ravel()
    return [int(c[s:s + TILE].sum()) for s in range(0, c.size, TILE)]


def write_frame(w, h, n_fill, hole_x=None, first=0):
    d = np.zeros(w * h, dtype=np.uint16)
    d[first:n_fill] = WRITE_DEPTH
    d = d.reshape(h, w)
    if hole_x is not None:
        d[2, hole_x] = 0
    return d


@functools.lru_cache(maxsize=None)
def write_frames(w, h, seed=7):
    """{count: depth (h, w)} with tile 0 of the frame emitting exactly `count` triangles (the full tile: every pixel filled), plus
    "tile1": tile 0 empty, tile 1 not.  A seeded search over how many pixels are filled in raster order and where one hole goes in row 2,
    the first row that emits: filling alone reaches only odd counts inside a row; a hole there takes three triangles away (five once
    row 3 is filled) and so changes the parity."""
    rng = np.random.default_rng(seed)
    holes = [None] + [int(x) for x in rng.permutation(np.arange(2, w - 3))[:5]]
    out = {}
    full = write_frame(w, h, w * h)
    out["full"] = full
    wanted = [c for c in WRITE_COUNTS if c != "full"]
    assert tile_counts(full)[0] > max(wanted)
    for n_fill in range(0, w * h + 1):
        if len(out) == len(WRITE_COUNTS):
            break
        for hx in holes:
            d = write_frame(w, h, n_fill, hx)
            c = tile_counts(d)[0]
            if c in wanted and c not in out:
                out[c] = d
    assert len(out) == len(WRITE_COUNTS), sorted(k for k in out if k != "full")
    out["tile1"] = write_frame(w, h, w * h, first=TILE + w)
    t = tile_counts(out["tile1"])
    assert t[0] == 0 and t[1] > 0
    for d in out.values():
        d.setflags(write=False)
    return out


def frame_of(name, depth, box=WIDE_BOX):
    f = Frame(name, depth.shape[1], depth.shape[0])
    f.depth, f.box = depth, box
    return f


def rig_of(frames, box=None):
    """A synth.Rig of the frames as sensors: identity pose, intrinsics(w, h), the first frame's box unless given."""
    from livescan3d_amd import synth
    return synth.Rig([f.depth for f in frames], [f.rgb() for f in frames], np.concatenate([intrinsics(f.w, f.h) for f in frames]),
                     np.concatenate([POSE] * len(frames)), frames[0].box if box is None else box)


def p2v_of(orc, f):
    """The frame's pixel -> vertex map as the oracle's createVertices leaves it under the frame's box."""
    return orc.create_vertices(f.depth, f.rgb(), intrinsics(f.w, f.h), POSE, f.box, want_maps=True)[2]


def write_pass_frames():
    """[Frame] of every searched write-pass frame of both sizes, named write<w>x<h>_<count>."""
    return [frame_of(f"write{w}x{h}_{k}", d) for w, h in WRITE_SIZES for k, d in write_frames(w, h).items()]


def fixture_frames():
    """What tests/golden/tri_boundary_ref.npz pins to the reference's own code: the general frame with both backgrounds, the special
    stencils under the wide box at both widths, the write-pass frames."""
    g = general_frame()
    return [g.with_background("holes"), g.with_background("dense"), hand_frame(64), hand_frame(61)] + write_pass_frames()
