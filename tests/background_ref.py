"""Background subtraction as include/NativeUtils.h defines it, restated in numpy (int64 throughout).  The GPU tests hold the kernels to this
file bit for bit; tests/test_background_ref.py holds this file to a plain-Python loop and a flood fill.

Per tick one u16 map per sensor (mm, 0 = no sample).  Model: one u16 per pixel of one tick, `lo`, the smallest non-zero sample seen while
learning (0: none).  learn -> classify -> blobs -> six counts per (tick, frame).  The blob rule is written without any union-find: every
kept pixel starts with its own raster index and takes the minimum over its kept 4-neighbours until nothing changes."""
import numpy as np

FOREGROUND, UNKNOWN, BACKGROUND, COMPONENTS, COMPONENTS_REMOVED, PIXELS_REMOVED = range(6)


def sensor_slices(widths, heights):
    """Where each sensor's pixels lie inside one tick's packed maps."""
    out, at = [], 0
    for w, h in zip(widths, heights):
        out.append(slice(at, at + w * h))
        at += w * h
    return out


def learn(model, maps):
    """model [pixels] u16, maps [T, pixels] u16 -> model'.  lo' = c if lo == 0 else min(lo, c) for c != 0."""
    lo = np.asarray(model, np.int64).copy()
    for c in np.asarray(maps, np.int64).reshape(-1, lo.size):
        take = (c != 0) & ((lo == 0) | (c < lo))
        lo[take] = c[take]
    return lo.astype(np.uint16)


def classify(maps, model, margin, rel_q, strict=True, floor=True):
    """-> (out [T, pixels] u16, foreground mask, unknown mask, background mask).  The two switches are the mutants of the test file."""
    c = np.asarray(maps, np.int64)
    lo = np.asarray(model, np.int64)[None, :]
    thr = margin + ((lo * rel_q) // 1024 if floor else -((-lo * rel_q) // 1024))
    sample = c != 0
    unknown = sample & (lo == 0)
    fore = sample & (lo != 0) & ((c + thr < lo) if strict else (c + thr <= lo))
    kept = unknown | fore
    return np.where(kept, c, 0).astype(np.uint16), fore, unknown, sample & ~kept


def labels_2d(mask, connectivity=4, highest=False):
    """mask [h, w] bool -> int64 [h, w]: the lowest raster index of each kept pixel's component (-1 where not kept), by iterated neighbour
    minima to a fixed point.  (Between two rounds every pixel also takes the value of the pixel its value names: that pixel lies in the
    same component, so nothing but the number of rounds changes.)"""
    h, w = mask.shape
    big = h * w
    idx = np.arange(big, dtype=np.int64).reshape(h, w)
    if highest:
        return np.where(mask, big - 1 - labels_2d(mask[::-1, ::-1], connectivity)[::-1, ::-1], -1)
    lab = np.where(mask, idx, big)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    while True:
        new = lab.copy()
        for dy, dx in steps:
            a = new[dy:, max(dx, 0):w + min(dx, 0)]           # the pixel further down / right ...
            b = new[:h - dy, max(-dx, 0):w - max(dx, 0)]      # ... and its neighbour up / left (views of `new`)
            m = np.where((a < big) & (b < big), np.minimum(a, b), big)     # (a fresh array: the two writes below only ever lower)
            np.minimum(a, m, out=a)
            np.minimum(b, m, out=b)
        flat = new.ravel()
        kept = flat < big
        flat[kept] = np.minimum(flat[kept], flat[flat[kept]])
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1)


def blobs(out, widths, heights, min_pixels, connectivity=4, at_least=True, highest=False):
    """out [T, pixels] u16 (non-zero = kept) -> (out', labels [T, pixels] int64 (frame-local raster index, -1: not kept), counts [T, n, 3]:
    components, components removed, pixels removed)."""
    out = np.asarray(out).copy()
    T = out.shape[0]
    lab_all = np.full(out.shape, -1, np.int64)
    counts = np.zeros((T, len(widths), 3), np.int64)
    for t in range(T):
        for f, (sl, w, h) in enumerate(zip(sensor_slices(widths, heights), widths, heights)):
            mask = (out[t, sl] != 0).reshape(h, w)
            lab = labels_2d(mask, connectivity, highest).ravel()
            lab_all[t, sl] = lab
            size = np.bincount(lab[lab >= 0], minlength=w * h)
            roots = np.flatnonzero(size)
            small = size < min_pixels if at_least else size <= min_pixels
            gone = (lab >= 0) & small[np.maximum(lab, 0)]
            frame = out[t, sl]
            frame[gone] = 0
            counts[t, f] = (roots.size, int(small[roots].sum()), int(gone.sum()))
    return out, lab_all, counts


def run(maps, model, widths, heights, margin, rel_q, min_pixels, **mutant):
    """One lsnFusionBackground: maps [T, pixels] u16 against model [pixels] u16 -> (out [T, pixels] u16, counts [T, n, 6] int64, labels or
    None).  `mutant`: switches of classify() / blobs(), for the test file's mutants only."""
    maps = np.asarray(maps, np.uint16)
    cm = {k: v for k, v in mutant.items() if k in ("strict", "floor")}
    bm = {k: v for k, v in mutant.items() if k in ("connectivity", "at_least", "highest")}
    out, fore, unknown, back = classify(maps, model, margin, rel_q, **cm)
    counts = np.zeros((maps.shape[0], len(widths), 6), np.int64)
    for f, sl in enumerate(sensor_slices(widths, heights)):
        counts[:, f, FOREGROUND] = fore[:, sl].sum(axis=1)
        counts[:, f, UNKNOWN] = unknown[:, sl].sum(axis=1)
        counts[:, f, BACKGROUND] = back[:, sl].sum(axis=1)
    labels = None
    if min_pixels >= 2:
        out, labels, c3 = blobs(out, widths, heights, min_pixels, **bm)
        counts[:, :, 3:] = c3
    return out, counts, labels


def run_packed(depth_maps_u8, model, widths, heights, margin, rel_q, min_pixels):
    """One host-export call (one tick) on the caller's packed uint8 view of the u16 maps -> (the maps as uint8, counts [n, 6])."""
    maps = np.ascontiguousarray(depth_maps_u8).view("<u2").reshape(1, -1)
    out, counts, _ = run(maps, model, widths, heights, margin, rel_q, min_pixels)
    return out.astype("<u2").view(np.uint8).ravel(), counts[0]


def learn_packed(model, depth_maps_u8):
    return learn(model, np.ascontiguousarray(depth_maps_u8).view("<u2").reshape(1, -1))
