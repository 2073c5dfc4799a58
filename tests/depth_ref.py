"""The two restatements of the reference's host code that several test modules share, unchanged from where they were written:
numpy_create_vertices (createVertices, src/NativeUtils/depthprocessing.cpp:122-187; tests/test_oracle_depth.py) and py_radial
(depthMapAndColorRadialCorrection, depthprocessing.cpp:191-261; tests/test_oracle_radial.py).  tests/test_export_pin.py holds both to the
reference's own exports."""
import numpy as np

VDT = [("R", "u1"), ("G", "u1"), ("B", "u1"), ("A", "u1"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")]


def numpy_create_vertices(depth, rgb, intr, wt, bounds):
    """numpy float32, one rounding per operation, same order as depthprocessing.cpp:149-163."""
    f = np.float32
    h, w = depth.shape
    cx, cy, fx, fy = [f(v) for v in intr[:4]]
    t = [f(v) for v in wt[:3]]
    R = np.asarray(wt[3:12], dtype=np.float32).reshape(3, 3)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        Z = depth.astype(np.float32) / f(1000.0)
        X = (x.astype(np.float32) - cx) / fx
        Y = (cy - y.astype(np.float32)) / fy
        X = X * Z
        Y = Y * Z
        X = X + t[0]
        Y = Y + t[1]
        Z = Z + t[2]
        ox = (X * R[0, 0] + Y * R[0, 1]) + Z * R[0, 2]
        oy = (X * R[1, 0] + Y * R[1, 1]) + Z * R[1, 2]
        oz = (X * R[2, 0] + Y * R[2, 1]) + Z * R[2, 2]
        b = np.asarray(bounds, dtype=np.float32)
        rejected = (ox < b[0]) | (ox > b[3]) | (oy < b[1]) | (oy > b[4]) | (oz < b[2]) | (oz > b[5])
    keep = (depth != 0) & ~rejected
    out = np.zeros(int(keep.sum()), dtype=VDT)
    out["R"], out["G"], out["B"] = rgb[keep][:, 0], rgb[keep][:, 1], rgb[keep][:, 2]
    out["A"] = 255
    out["X"], out["Y"], out["Z"] = ox[keep], oy[keep], oz[keep]
    return out


def np_warp_target(w, h, intr):
    """The warp target of every pixel of a w x h frame (depthprocessing.cpp:205-213: u, v, r, d, (int)), vectorised in float32 with one
    rounding per operation and the cvttss2si rule of py_radial's f2i.  Returns int64 (h * w): the destination pixel x_corr + y_corr * w of
    source pixel x + y * w, -1 where the target lies outside the frame.  It does not depend on the depth values."""
    f = np.float32
    cx, cy, fx, fy, r2, r4, r6 = [f(v) for v in intr]
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    with np.errstate(all="ignore"):
        u = (x.astype(f) - cx) / fx
        v = (y.astype(f) - cy) / fy
        r = u * u + v * v
        d = f(1) - r2 * r - r4 * r * r - r6 * r * r * r
        xf = u * d * fx + cx
        yf = v * d * fy + cy

        def f2i(a):
            ok = (a > f(-2147483904.0)) & (a < f(2147483648.0))     # NaN / out of range: cvttss2si -> INT_MIN
            return np.where(ok, np.trunc(np.where(ok, a, f(0))).astype(np.int64), -2147483648)

        xc, yc = f2i(xf), f2i(yf)
    inside = (xc >= 0) & (xc < w) & (yc >= 0) & (yc < h)
    return np.where(inside, xc + yc * w, -1).ravel()


def py_radial(depth2d, rgb3, intr):
    f = np.float32
    h, w = depth2d.shape
    cx, cy, fx, fy, r2, r4, r6 = [f(v) for v in intr]
    depth = depth2d.ravel()
    colors = rgb3.reshape(-1, 3)
    map_copy = np.zeros(w * h, np.uint16)
    colors_copy = np.zeros((w * h, 3), np.uint8)

    def f2i(v):
        if not (v > f(-2147483904.0) and v < f(2147483648.0)):   # NaN / out of range: cvttss2si -> INT_MIN
            return -2147483648
        return int(np.trunc(v))

    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if depth[x + y * w] == 0:
                    continue
                u = (f(x) - cx) / fx
                v = (f(y) - cy) / fy
                r = u * u + v * v
                d = f(1) - r2 * r - r4 * r * r - r6 * r * r * r
                xc = f2i(u * d * fx + cx)
                yc = f2i(v * d * fy + cy)
                if 0 <= xc < w and 0 <= yc < h:
                    map_copy[xc + yc * w] = depth[x + y * w]
                    colors_copy[xc + yc * w] = colors[x + y * w]
    shifts = [-w - 1, -w, -w + 1, -1, 1, w - 1, w, w + 1]
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            pos = x + y * w
            if map_copy[pos] != 0:
                continue
            n = s = 0
            sc = [0, 0, 0]
            prev = -1
            for sh in shifts:
                mv = int(map_copy[pos + sh])
                if mv > 0 and (prev == -1 or abs(mv - prev) < 30):
                    prev = mv
                    n += 1
                    s += mv
                    for c in range(3):
                        sc[c] += int(colors_copy[pos + sh, c])
            if n > 4:
                map_copy[pos] = s // n
                for c in range(3):
                    colors_copy[pos, c] = sc[c] // n
    return map_copy.reshape(h, w), colors_copy.reshape(h, w, 3)
