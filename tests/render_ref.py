"""CPU restatement of the render stage (lsnFusionRenderViews).  TEST INFRASTRUCTURE ONLY.

The reference has no renderer (its merged mesh goes to an OpenGL window), so the stage is defined, not copied; what it is built from
is the reference's and pinned elsewhere: pointProjection with the inverted pose (color_ref.project, tests/test_merge_ref.py), and
drawTriangle's set-up, fill rule, weights and depth value (merge_ref.triangle_setup / triangle_pixels, pinned to the reference's own
drawTriangle through tests/golden/overlay_merge_ref.npz).  Here, in numpy:

  vertex     project() -> integer (x, y), d in mm clamped to [0, 65535]; drawable iff 0 <= x < w, 0 <= y < h and d != 0
  mesh       a triangle is drawn iff its indices are in range and its three vertices are drawable (no clipping); candidates are the
             pixels drawTriangle covers with their val, val == 0 skipped; per pixel the smallest (val, triangle index) wins; depth =
             val, colour per channel = trunc(((c1 w1 + c2 w2) + c3 w3) + 0.5f) in float32, clamped to [0, 255]
  points     every drawable vertex is a candidate (d, vertex index) at its pixel; the colour is its own
  empty      depth 0, colour 0, 0, 0

tests/test_render_ref.py ties the z-buffer rule to the reference's own depth maps."""
import numpy as np

from tests import color_ref, merge_ref

f32 = np.float32
MAX_SIDE = 1024
MAX_VIEWS = 16
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], dtype=np.float32)


def walk(s):
    """merge_ref.triangle_pixels with the weights: every covered (triangle, pixel) of the set-up `s`.  Returns (k, x, y, val, w1, w2, w3).
    Asserts that no 28.4 fixed-point value leaves int32 (true for every view of at most 1024 x 1024)."""
    bw = np.maximum(s["maxx"] - s["minx"], 0)
    bh = np.maximum(s["maxy"] - s["miny"], 0)
    cnt = np.where(s["den"] != 0, bw * bh, 0)                                            # den == 0: no pixel (:662-663)
    k = np.repeat(np.arange(len(cnt)), cnt)
    j = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    bwk = np.maximum(bw[k], 1)
    px = s["minx"][k] + j % bwk
    py = s["miny"][k] + j // bwk
    inside = np.ones(len(k), dtype=bool)
    for c, DX, DY in s["C"]:
        parts = (c[k], DX[k] * (16 * py), DY[k] * (16 * px), c[k] + DX[k] * (16 * py) - DY[k] * (16 * px))
        assert all(np.all(np.abs(p) < 2 ** 31) for p in parts), "a 28.4 product left int32"
        inside &= parts[3] >= 0                                                          # :648-650, :697-703
    k, px, py = k[inside], px[inside], py[inside]
    fden = s["den"][k].astype(f32)
    dx3, dy3 = (px - s["x3"][k]).astype(f32), (py - s["y3"][k]).astype(f32)
    term21, term22 = s["x32"][k] * dy3, s["x13"][k] * dy3                              # :671-672
    w1 = (s["y23"][k] * dx3 + term21) / fden                                            # :677
    w2 = (s["y31"][k] * dx3 + term22) / fden                                            # :678
    w3 = f32(1.0) - w1 - w2                                                             # :679
    fd1, fd2, fd3 = (f[k] for f in s["fd"])
    val = merge_ref.cvt_u16_x64(fd1 * w1 + fd2 * w2 + fd3 * w3)                         # :682
    return k, px, py, val, w1, w2, w3


def project_view(verts, intr7, wt12, w, h):
    """(x, y, d, drawable) of every vertex in the view."""
    with np.errstate(invalid="ignore"):      # (a NaN or an inf in a vertex: the conversion gives INT_MIN)
        x, y, d = color_ref.project(verts["X"], verts["Y"], verts["Z"], intr7, wt12)
    return x, y, d, (x >= 0) & (x < w) & (y >= 0) & (y < h) & (d != 0)


def render(verts, tris, intr7, wt12, w, h, labels=None, terms=None):
    """One view of one tick.  verts: VERTEX_DTYPE; tris: (m, 3) vertex indices, or None for points; labels: the triangles' indices
    (default 0 .. m-1: their positions).  Returns (depth u16 (h, w), rgb u8 (h, w, 3), {"drawn", "pixels", "boxes"}).
    terms: a list that receives one record of the intermediate values (what the witnesses of tests/test_render_boundary_ref.py read):
    x, y, d, ok per vertex; in mesh mode keep per triangle, den per kept triangle, every candidate (ck its triangle, cx, cy, cval,
    cw1, cw2, cw3; val 0 included), and per winning pixel wp (y * w + x), wk (its triangle) and v (the three float32 colour sums, the
    0.5 not yet added)."""
    assert 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE
    nv = len(verts)
    x, y, d, ok = project_view(verts, intr7, wt12, w, h)
    col = np.stack([verts["R"], verts["G"], verts["B"]], axis=1).astype(f32) if nv else np.zeros((0, 3), f32)
    none = np.iinfo(np.int64).max
    key = np.full(w * h, none, dtype=np.int64)
    depth = np.zeros(w * h, dtype=np.uint16)
    rgb = np.zeros((w * h, 3), dtype=np.uint8)
    info = {"drawn": 0, "pixels": 0, "boxes": np.zeros(0, np.int64)}
    rec = {"x": x, "y": y, "d": d, "ok": ok}
    if tris is None:
        g = np.flatnonzero(ok)
        p = y[g] * w + x[g]
        np.minimum.at(key, p, (d[g] << 32) | g)
        won = key != none
        depth[won] = key[won] >> 32
        rgb[won] = col[key[won] & 0xFFFFFFFF].astype(np.uint8)
        info["drawn"] = len(g)
    else:
        tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
        labels = np.arange(len(tris)) if labels is None else np.asarray(labels, dtype=np.int64)
        inr = np.all((tris >= 0) & (tris < nv), axis=1)
        keep = inr.copy()
        keep[inr] = np.all(ok[tris[inr]], axis=1)
        t, lab = tris[keep], labels[keep]
        info["drawn"] = int(keep.sum())
        rec.update(keep=keep, den=np.zeros(0, np.int64), wp=np.zeros(0, np.int64), wk=np.zeros(0, np.int64), v=np.zeros((0, 3), f32),
                   **{c: np.zeros(0, np.int64) for c in ("ck", "cx", "cy", "cval")}, **{c: np.zeros(0, f32) for c in ("cw1", "cw2", "cw3")})
        if len(t):
            i1, i2, i3 = t[:, 0], t[:, 1], t[:, 2]
            s = merge_ref.triangle_setup(x[i1], y[i1], d[i1], x[i2], y[i2], d[i2], x[i3], y[i3], d[i3])
            info["boxes"] = np.where(s["den"] != 0, (s["maxx"] - s["minx"]) * (s["maxy"] - s["miny"]), 0)
            k, px, py, val, w1, w2, w3 = walk(s)
            rec.update(den=s["den"], ck=lab[k], cx=px, cy=py, cval=val, cw1=w1, cw2=w2, cw3=w3)
            seen = val != 0                                                              # candidates of val 0 are skipped
            k, px, py, val, w1, w2, w3 = (a[seen] for a in (k, px, py, val, w1, w2, w3))
            p = py * w + px
            cand = (val << 32) | lab[k]
            np.minimum.at(key, p, cand)
            win = cand == key[p]                                                         # one candidate per pixel: labels are distinct
            k, p, w1, w2, w3 = k[win], p[win], w1[win], w2[win], w3[win]
            assert len(np.unique(p)) == len(p)
            depth[p] = key[p] >> 32
            c1, c2, c3 = col[i1[k]], col[i2[k]], col[i3[k]]
            v0 = (c1 * w1[:, None] + c2 * w2[:, None]) + c3 * w3[:, None]
            v = v0 + f32(0.5)
            assert v.dtype == f32
            rgb[p] = np.clip(np.trunc(v), 0, 255).astype(np.uint8)
            rec.update(wp=p, wk=lab[k], v=v0)
    info["pixels"] = int((depth != 0).sum())
    if terms is not None:
        terms.append(rec)
    return depth.reshape(h, w), rgb.reshape(h, w, 3), info


def render_views(verts, tris, intr, wt, w, h):
    """Several views (7 / 12 floats each) of one tick.  Returns (depth (V, h, w), rgb (V, h, w, 3), [info])."""
    intr, wt = np.asarray(intr, f32).reshape(-1, 7), np.asarray(wt, f32).reshape(-1, 12)
    assert 1 <= len(intr) <= MAX_VIEWS and len(intr) == len(wt)
    out = [render(verts, tris, intr[v], wt[v], w, h) for v in range(len(intr))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out]


def vertices_at(xyd, intr7, colors=None):
    """Vertices (VERTEX_DTYPE-like structured array) that project exactly onto the integer (x, y, d) rows of `xyd` under the identity
    pose: Z = (d + 0.5) / 1000, X = (x - cx) Z / fx, Y = (cy - y) Z / fy.  Asserted through color_ref.project."""
    xyd = np.asarray(xyd, dtype=np.int64).reshape(-1, 3)
    cx, cy, fx, fy = (float(v) for v in np.asarray(intr7, dtype=f32)[:4])
    Z = (xyd[:, 2] + 0.5) / 1000.0
    v = np.zeros(len(xyd), dtype=[("R", "u1"), ("G", "u1"), ("B", "u1"), ("A", "u1"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4")])
    v["X"], v["Y"], v["Z"], v["A"] = (xyd[:, 0] - cx) * Z / fx, (cy - xyd[:, 1]) * Z / fy, Z, 255
    if colors is not None:
        c = np.asarray(colors).reshape(-1, 3)
        v["R"], v["G"], v["B"] = c[:, 0], c[:, 1], c[:, 2]
    x, y, d = color_ref.project(v["X"], v["Y"], v["Z"], intr7, IDENTITY)
    assert np.array_equal(x, xyd[:, 0]) and np.array_equal(y, xyd[:, 1]) and np.array_equal(d, xyd[:, 2])
    return v


def soup(tris9, intr7, colors=None):
    """A triangle soup from drawTriangle-style rows {x1, y1, d1, x2, y2, d2, x3, y3, d3}: three vertices of its own per triangle.
    Returns (vertices, triangles (m, 3))."""
    t9 = np.asarray(tris9, dtype=np.int64).reshape(-1, 9)
    return vertices_at(t9.reshape(-1, 3), intr7, colors), np.arange(3 * len(t9), dtype=np.int32).reshape(-1, 3)


def intrinsics(w, h, f=None):
    """A view's 7 floats: the principal point at the centre, focal length f (default: the width)."""
    f = float(w if f is None else f)
    return np.array([w / 2.0, h / 2.0, f, f, 0, 0, 0], dtype=f32)


# Intrinsics under which a 96 x 80 ring rig still lands in a 1 x 1 view (everything left of the axis falls into the one pixel) and in a
# 1024 x 3 view (zoomed 8x along x, squeezed along y so that whole triangles fit the three rows: there is no clipping).
TINY_INTR = {(1, 1): np.array([0.5, 0.5, 0.4, 0.4, 0, 0, 0], dtype=f32), (1024, 3): np.array([512, 1.5, 750, 20, 0, 0, 0], dtype=f32)}


def pose_between(wt_a, wt_b, s=0.5):
    """A pose between two sensors' world transforms (12 floats: t, R row-major; p_world = R (p_cam + t)): the camera centre and the
    rotation interpolated, the rotation re-orthonormalised by an SVD."""
    a, b = np.asarray(wt_a, np.float64), np.asarray(wt_b, np.float64)
    Ra, Rb = a[3:].reshape(3, 3), b[3:].reshape(3, 3)
    ca, cb = Ra @ a[:3], Rb @ b[:3]                       # the camera centres in the world
    U, _, Vt = np.linalg.svd((1 - s) * Ra + s * Rb)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1, 1, -1]) @ Vt
    c = (1 - s) * ca + s * cb
    return np.concatenate([R.T @ c, R.ravel()]).astype(f32)


def pose_at(R, centre):
    """The 12 floats of a camera with rotation R (camera -> world) whose centre is at `centre` (world)."""
    R = np.asarray(R, np.float64)
    return np.concatenate([R.T @ np.asarray(centre, np.float64), R.ravel()]).astype(f32)


def ring_views(rig):
    """Four views of a ring rig, 12 floats each: sensor 0's own pose, a pose between sensors 0 and 1 (sensor 0 again when it is alone), a
    pose inside the scene (0.7 m from the centre, the floor partly behind it), sensor 0's place looking away from the scene."""
    wt = np.asarray(rig.wt, f32).reshape(-1, 12)
    R0 = wt[0, 3:].reshape(3, 3).astype(np.float64)
    c0 = R0 @ wt[0, :3].astype(np.float64)
    turn = np.array([[-1, 0, 0], [0, 1, 0], [0, 0, -1]], dtype=np.float64)   # Ry(pi)
    return np.stack([wt[0], pose_between(wt[0], wt[min(1, len(wt) - 1)]), pose_at(R0, 0.35 * c0), pose_at(R0 @ turn, c0)])
