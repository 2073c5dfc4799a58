"""Numpy restatement of LiveScanClient's flying-pixel filter (KinectCapture::filterFlyingPixels with three arguments,
src/LiveScanClient/kinectCapture.cpp:132-174), the definition flying.hip implements.  Held to the reference's
own code bit for bit by tests/test_flying_ref.py through tests/golden/flying_pixels_ref.npz.

One u16 depth map w x h, neighbourhood r, threshold thr:
  * N = (2r+1)^2 - 1 neighbours, the full window without its centre;
  * pixels with r <= x < w - r and r <= y < h - r are examined, the border band of width r is never changed (a frame with 2r+1 > w or
    > h is left as it is);
  * an examined pixel (value 0 included) is removed iff MORE than N / 2 (integer division) of its neighbours differ from it by MORE
    than thr; a neighbour of depth 0 counts like any other value;
  * every decision is taken on the unmodified map; removed pixels become 0.
The reference's third argument (maxNonFittingNeighbours) is overwritten with N / 2 before it is read, so it is no parameter here.
r <= 0 means off (defined here: the reference does nothing for r in {-1, 0} and reads out of bounds below that)."""
import numpy as np


def removed_mask(depth, r, thr):
    """bool [h, w]: the pixels the filter decides to remove (whatever their value; a removed pixel of depth 0 stays 0)."""
    d = np.asarray(depth)
    assert d.ndim == 2
    h, w = d.shape
    out = np.zeros((h, w), dtype=bool)
    r = int(r)
    if r <= 0 or 2 * r + 1 > w or 2 * r + 1 > h:
        return out
    # the reference compares int diffs against (float)thr; |diff| <= 65535 is exact in float, so for an int thr this is the int comparison
    thr = int(thr)
    v = d.astype(np.int64)
    c = v[r:h - r, r:w - r]
    n_diff = np.zeros(c.shape, dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            n_diff += np.abs(v[r + dy:h - r + dy, r + dx:w - r + dx] - c) > thr
    n = (2 * r + 1) ** 2 - 1
    out[r:h - r, r:w - r] = n_diff > n // 2
    return out


def filter(depth, r, thr):
    """The filtered map (a new u16 array [h, w])."""
    d = np.array(depth, dtype=np.uint16, copy=True)
    d[removed_mask(d, r, thr)] = 0
    return d


def removed_count(depth, r, thr):
    """Pixels of depth != 0 the filter sets to 0 (what lsnFusionFlyingDiagnostics reports per sensor)."""
    d = np.asarray(depth)
    return int((removed_mask(d, r, thr) & (d != 0)).sum())


def filter_packed(depth_maps, widths, heights, r, thr):
    """The filter on every frame of a call's packed depth array (uint8 view of little-endian u16, KinectServer.cs:453-498).
    Returns (filtered packed uint8 array, removed count per sensor)."""
    dm = np.ascontiguousarray(depth_maps).view(np.uint8).view("<u2").copy()
    removed, p = [], 0
    for w, h in zip(np.asarray(widths).tolist(), np.asarray(heights).tolist()):
        f = dm[p:p + w * h].reshape(h, w)
        removed.append(removed_count(f, r, thr))
        dm[p:p + w * h] = filter(f, r, thr).ravel()
        p += w * h
    return dm.view(np.uint8), np.array(removed, dtype=np.int32)


def filter_in_place_sequential(depth, r, thr):
    """NOT the filter: the variant that zeroes as it scans (decisions see the pass's own zeros).  The fixture generator uses it to
    prove that a case tells the two apart."""
    d = np.array(depth, dtype=np.int64, copy=True)
    h, w = d.shape
    n = (2 * r + 1) ** 2 - 1
    if r <= 0 or 2 * r + 1 > w or 2 * r + 1 > h:
        return d.astype(np.uint16)
    for y in range(r, h - r):
        for x in range(r, w - r):
            win = d[y - r:y + r + 1, x - r:x + r + 1]
            if int((np.abs(win - d[y, x]) > int(thr)).sum()) > n // 2:
                d[y, x] = 0
    return d.astype(np.uint16)
