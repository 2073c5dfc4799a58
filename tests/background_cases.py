"""Hand-made cases and the seeded generator for background subtraction (tests/background_ref.py is the definition).  Every case carries a
witness: an assertion on the restatement's own result that the case reaches what it is named for.  tests/test_background_ref.py runs the
witnesses on the CPU; the GPU tests run the same cases against the kernels."""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from tests import background_ref as ref

TILE_W, TILE_H = 128, 16


@dataclass
class Case:
    name: str
    sizes: list              # [(w, h)] per sensor
    maps: np.ndarray         # [T, pixels] u16
    model: np.ndarray        # [pixels] u16
    params: tuple            # (margin, rel_q, min_pixels)
    witness: Callable        # (out, counts, labels) of ref.run -> None, asserting

    @property
    def widths(self):
        return [s[0] for s in self.sizes]

    @property
    def heights(self):
        return [s[1] for s in self.sizes]

    def want(self, **mutant):
        return ref.run(self.maps, self.model, self.widths, self.heights, *self.params, **mutant)


def thr_of(lo, margin, rel_q):
    return margin + (lo * rel_q) // 1024


# ---- classification: single rows, the model and the samples written out ------------------------------------------------------------------

def _classify_case(name, margin, rel_q, los):
    """For every model value lo of `los`: the samples c with c + thr == lo + 1, == lo (both background) and == lo - 1 (foreground) where they
    exist, and 65535, 1 and 0."""
    lo_l, c_l = [], []
    for lo in los:
        thr = thr_of(lo, margin, rel_q)
        for c in (lo - thr + 1, lo - thr, lo - thr - 1, 65535, 1, 0):
            if 0 <= c <= 65535:
                lo_l.append(lo)
                c_l.append(c)
    model, maps = np.array(lo_l, np.uint16), np.array([c_l], np.uint16)

    def witness(out, counts, labels):
        lo, c = model.astype(np.int64), maps[0].astype(np.int64)
        thr = margin + (lo * rel_q) // 1024
        edge = (lo != 0) & (c != 0)
        for d, kept in ((0, False), (-1, True)):                    # c + thr == lo is background, == lo - 1 foreground
            at = edge & (c + thr == lo + d)
            assert at.any() or not (lo > thr + 1).any(), name
            assert ((out[0][at] != 0) == kept).all(), name
        assert ((out[0] == maps[0]) | (out[0] == 0)).all()
        assert (out[0][(lo == 0) & (c != 0)] != 0).all()            # unknown: kept
    return Case(name, [(len(lo_l), 1)], maps, model, (margin, rel_q, 0), witness)


def classify_cases():
    out = [
        # lo * 8 on both sides of a multiple of 1024: 2047 * 8 = 16376 (15.99), 2048 * 8 = 16 * 1024, 2049 * 8 = 16392
        _classify_case("threshold_floor_at_multiples_of_1024", 20, 8, [2047, 2048, 2049, 127, 128, 129, 1000]),
        _classify_case("rel_q_0", 20, 0, [21, 22, 500, 65535, 0, 1]),
        _classify_case("rel_q_255", 1, 255, [1, 2, 4, 5, 4096, 4097, 65535, 0]),
        _classify_case("margin_4095", 4095, 3, [4095, 4096, 4097, 5000, 65535, 0, 1]),
        _classify_case("margin_4095_rel_q_255", 4095, 255, [65535, 30000, 5500, 5600, 0]),
    ]
    # thr without the floor: lo = 2047, rel_q = 8 gives 15.99; a sample at lo - (margin + 15) - 1 is foreground only with the floor
    c = out[0]
    assert (c.want()[0] != c.want(floor=False)[0]).any() and (c.want()[0] != c.want(strict=False)[0]).any()
    return out


# ---- blobs: masks; the model is empty, so every sample is unknown and kept by classification ---------------------------------------------

def _mask_case(name, masks, min_pixels, witness, ticks=1):
    """masks: per tick a list of [h, w] bool arrays (one per sensor), or one such list for every tick."""
    per_tick = masks if isinstance(masks[0], list) else [masks] * ticks
    sizes = [(m.shape[1], m.shape[0]) for m in per_tick[0]]
    maps = np.stack([np.concatenate([np.where(m, 1000 + 7 * i, 0).ravel() for i, m in enumerate(ms)]) for ms in per_tick]).astype(np.uint16)
    return Case(name, sizes, maps, np.zeros(maps.shape[1], np.uint16), (50, 4, min_pixels), witness)


def _one_component(first_index, size=None, frame=0):
    def witness(out, counts, labels):
        assert counts[0, frame, ref.COMPONENTS] == 1 and counts[0, frame, ref.COMPONENTS_REMOVED] == 0
        kept = labels[0] >= 0
        assert kept.any() and (labels[0][kept] == first_index).all()
        if size is not None:
            assert int(kept.sum()) == size
    return witness


def tiles_touched(mask):
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    return {(int(y) // TILE_H, int(x) // TILE_W) for y, x in zip(ys, xs)}


def serpentine(w, h):
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for k, y in enumerate(range(1, h - 1, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(w, h):
    """A rectangular spiral, one corridor a pixel wide with a free pixel between its turns, from the frame's corner inwards."""
    m = np.zeros((h, w), bool)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = True
    turns = 0
    while turns < 2:
        nx, ny, ax, ay = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 0 <= nx < w and 0 <= ny < h and not m[ny, nx] and not (0 <= ax < w and 0 <= ay < h and m[ay, ax]):
            x, y, turns = nx, ny, 0
            m[y, x] = True
        else:
            dx, dy, turns = -dy, dx, turns + 1
    return m


def blob_cases():
    cases = []
    # sizes min_pixels - 1, min_pixels, min_pixels + 1, in a frame below one chunk and in one that crosses tiles
    for w, h, mp in ((7, 5, 3), (136, 40, 9)):
        m = np.zeros((h, w), bool)
        m[0, 0:mp - 1] = True
        m[2, 0:mp] = True
        m[4, 0:mp + 1] = True
        if w > 128:
            m[:] = False
            m[3, 124:124 + mp - 1] = True                          # each bar across the tile edge at x = 128
            m[14:17, 126] = True                                   # ... and one across y = 16, three pixels
            m[20, 124:124 + mp] = True
            m[30, 124:124 + mp + 1] = True

        def witness(out, counts, labels, mp=mp, big=w > 128):
            assert counts[0, 0, ref.COMPONENTS] == (4 if big else 3)
            assert counts[0, 0, ref.COMPONENTS_REMOVED] == (2 if big else 1)
            assert counts[0, 0, ref.PIXELS_REMOVED] == mp - 1 + (3 if big else 0)
            assert int((out[0] != 0).sum()) == 2 * mp + 1
        cases.append(_mask_case(f"sizes_around_min_pixels_{w}x{h}", [m], mp, witness))
    # a component that meets another only at a tile CORNER (129 x 17: four tiles, the last column and row one pixel wide)
    m = np.zeros((17, 129), bool)
    m[15, 127] = m[16, 128] = True

    def corner(out, counts, labels):
        assert counts[0, 0, 3:].tolist() == [2, 2, 2] and not out.any()
    cases.append(_mask_case("corner_contact_is_not_joined", [m], 2, corner))
    # a U and a comb inside one tile: the arms' tops learn of each other only through the bottom
    u = np.zeros((16, 128), bool)
    u[0:11, 10] = u[0:11, 20] = True
    u[10, 10:21] = True
    cases.append(_mask_case("u_inside_a_tile", [u], 2, _one_component(10, 31)))
    comb = np.zeros((16, 128), bool)
    comb[15, 3:100] = True
    comb[2:16, 3:100:2] = True
    cases.append(_mask_case("comb_inside_a_tile", [comb], 2, _one_component(2 * 128 + 3)))
    # the deepest chains: one corridor through every tile of a 256 x 64 frame
    for name, m in (("serpentine_256x64", serpentine(256, 64)), ("spiral_256x64", spiral(256, 64))):
        assert len(tiles_touched(m)) == 8, name
        cases.append(_mask_case(name, [m], 2, _one_component(0, int(m.sum()))))
    cases.append(_mask_case("full_frame_136x40", [np.ones((40, 136), bool)], 5440, _one_component(0, 5440)))

    def full_removed(out, counts, labels):
        assert counts[0, 0, 3:].tolist() == [1, 1, 5440] and not out.any()
    cases.append(_mask_case("full_frame_one_short", [np.ones((40, 136), bool)], 5441, full_removed))

    def empty(out, counts, labels):
        assert not counts.any() and not out.any()
    cases.append(_mask_case("empty_frame", [np.zeros((17, 129), bool)], 2, empty))
    yy, xx = np.mgrid[0:40, 0:136]

    def checker(out, counts, labels):
        assert counts[0, 0, 3:].tolist() == [2720, 2720, 2720] and not out.any()
    cases.append(_mask_case("checkerboard", [(yy + xx) % 2 == 0], 2, checker))
    m = np.zeros((17, 129), bool)
    m[14:17, 126:129] = True
    cases.append(_mask_case("last_row_and_column_129x17", [m], 9, _one_component(14 * 129 + 126, 9)))
    m = np.zeros((1, 1), bool)
    m[0, 0] = True

    def single(out, counts, labels):
        assert counts[0, 0, 3:].tolist() == [1, 1, 1] and not out.any()
    cases.append(_mask_case("one_pixel_frame", [m], 2, single))
    # the end of a row and the start of the next are neighbours in memory, not in the image
    m = np.zeros((5, 7), bool)
    m[1, 5:7] = m[2, 0:2] = True

    def wrap(out, counts, labels):
        assert counts[0, 0, 3:].tolist() == [2, 2, 4]
    cases.append(_mask_case("row_ends_do_not_wrap", [m], 3, wrap))
    # two sensors of one width: the last row of the first and the first row of the second are neighbours in memory only
    a, b = np.zeros((5, 7), bool), np.zeros((5, 7), bool)
    a[4, 2:5] = b[0, 2:5] = True

    def frames(out, counts, labels):
        assert counts[0, :, 3:].tolist() == [[1, 1, 3], [1, 1, 3]]
    cases.append(_mask_case("frames_are_not_joined", [a, b], 4, frames))
    # ... and so are two ticks of one batch

    def ticks(out, counts, labels):
        assert counts[:, 0, 3:].tolist() == [[1, 1, 3], [1, 1, 3]]
    cases.append(_mask_case("ticks_are_not_joined", [[a], [b]], 4, ticks))
    # the same mask in two ticks of one batch, three sensors of different sizes
    rng = np.random.default_rng(11)
    masks = [blobby_mask(rng, w, h) for w, h in ((129, 17), (7, 5), (136, 40))]

    def twice(out, counts, labels):
        assert np.array_equal(out[0], out[1]) and np.array_equal(counts[0], counts[1])
        assert (counts[0, :, ref.COMPONENTS] > 0).all() and counts[0, :, ref.COMPONENTS_REMOVED].sum() > 0 and out.any()
    cases.append(_mask_case("same_mask_in_two_ticks_three_sensors", masks, 6, twice, ticks=2))
    return cases


def blobby_mask(rng, w, h, specks=0.03):
    """Rectangles that cross the frame's tile edges where it has any, and isolated specks."""
    m = rng.random((h, w)) < specks
    for _ in range(3):
        bw, bh = int(rng.integers(1, max(2, w // 3 + 1))), int(rng.integers(1, max(2, h // 2 + 1)))
        x0, y0 = int(rng.integers(0, w - bw + 1)), int(rng.integers(0, h - bh + 1))
        m[y0:y0 + bh, x0:x0 + bw] = True
    if w > TILE_W:
        m[h // 2, TILE_W - 3:min(w, TILE_W + 3)] = True
    if h > TILE_H:
        m[TILE_H - 2:TILE_H + 2, w // 3] = True
    return m


def cases():
    return classify_cases() + blob_cases()


# ---- learning ----------------------------------------------------------------------------------------------------------------------------

def learn_maps(rng, n_pixels, n_ticks):
    """[n_ticks, n_pixels] u16 of an empty room: a per-pixel depth with a few millimetres of noise, a fifth of the samples dropped, a
    twentieth of the pixels never seen, the extremes 1 and 65535 among the values."""
    base = rng.integers(600, 8000, n_pixels).astype(np.int64)
    base[rng.random(n_pixels) < 0.01] = 65535
    base[rng.random(n_pixels) < 0.01] = 5
    dead = rng.random(n_pixels) < 0.05
    maps = np.clip(base[None, :] + rng.integers(-4, 5, (n_ticks, n_pixels)), 1, 65535)
    maps[rng.random(maps.shape) < 0.2] = 0
    maps[:, dead] = 0
    return maps.astype(np.uint16)


# ---- the seeded generator ----------------------------------------------------------------------------------------------------------------

FUZZ_SEEDS = tuple(range(10))
FIRST_SIZES = [(136, 40), (256, 17), (129, 33), (264, 18)]         # the first sensor always has more than one tile


def fuzz_case(seed):
    """The seed's (sizes, params, room [2, pixels] (the ticks to learn from), maps [T, pixels]): 1..8 sensors -- the first of FIRST_SIZES, the
    others of support's rig sizes --, 1..5 ticks.  A room with unseen pixels, subjects in front of it (rectangles, one of them across a
    tile edge of the first sensor), specks, dropouts."""
    from tests import support
    rng = np.random.default_rng(23000 + seed)
    n = int(rng.integers(1, 9))
    sizes = [FIRST_SIZES[int(rng.integers(0, len(FIRST_SIZES)))]] + support.ragged_or_equal(140, 24, [8, 128, 136], [1, 16, 17])(rng, n)[1:]
    margin, rel_q = int(rng.choice([1, 20, 60, 4095])), int(rng.choice([0, 8, 64, 255]))
    min_pixels = int(rng.choice([0, 1, 2, 7, 40])) if seed % 5 else 12
    T = int(rng.integers(1, 6))
    px = sum(w * h for w, h in sizes)
    wall = rng.integers(9000, 30000, px).astype(np.int64)
    unseen = rng.random(px) < 0.04
    room = np.clip(wall[None, :] + rng.integers(-3, 4, (2, px)), 1, 65535)
    room[rng.random(room.shape) < 0.15] = 0
    room[:, unseen] = 0
    maps = np.clip(wall[None, :] + rng.integers(-3, 4, (T, px)), 1, 65535)
    for t in range(T):
        for f, sl in enumerate(ref.sensor_slices([s[0] for s in sizes], [s[1] for s in sizes])):
            w, h = sizes[f]
            m = blobby_mask(rng, w, h, specks=0.01)
            if f == 0:                                             # a subject across the first tile edge, more than 40 pixels
                m[max(0, h // 2 - 3):h // 2 + 3, TILE_W - 6:TILE_W + 6] = True
            frame = maps[t, sl]
            # far enough in front of the wall for every margin and rel_q of the generator: lo / 2 - 100 > 4095 + lo / 4
            frame[m.ravel()] = wall[sl][m.ravel()] // 2 - 100
    maps[rng.random(maps.shape) < 0.1] = 0
    return sizes, (margin, rel_q, min_pixels), room.astype(np.uint16), maps.astype(np.uint16)


def fuzz_witness(seed):
    """What test_background_ref.py asserts for every seed, so that the GPU test cannot pass on trivial inputs."""
    sizes, params, room, maps = fuzz_case(seed)
    widths, heights = [s[0] for s in sizes], [s[1] for s in sizes]
    model = ref.learn(np.zeros(maps.shape[1], np.uint16), room)
    out, counts, labels = ref.run(maps, model, widths, heights, *params)
    assert counts[:, :, ref.FOREGROUND].sum() > 0 and counts[:, :, ref.BACKGROUND].sum() > 0 and counts[:, :, ref.UNKNOWN].sum() > 0, seed
    # a component across two tiles: of the classified mask of the first sensor (whatever min_pixels is)
    first = (ref.classify(maps, model, *params[:2])[0][0, :widths[0] * heights[0]] != 0).reshape(heights[0], widths[0])
    lab = ref.labels_2d(first)
    spans = max(len(tiles_touched(lab == v)) for v in np.unique(lab[lab >= 0]))
    assert spans >= 2, seed
    if params[2] >= 2:
        assert counts[:, :, ref.COMPONENTS_REMOVED].sum() > 0, seed
        assert (counts[:, :, ref.COMPONENTS] - counts[:, :, ref.COMPONENTS_REMOVED]).sum() > 0 and out.any(), seed
    return params
