"""The DEFINITION of the colour blend across views (lsnFusionColorBlend, csrc/color_blend.hip), in numpy.
TEST INFRASTRUCTURE ONLY.  There is no reference for this stage: what is written here is what the kernels are held to, bit for bit.

Inputs: a rig's depth maps, the merged cloud fused from them (`verts`: as fused, or as another stage -- the colour transfer, a first
blend -- left it), depth_tol (mm) and min_confidence.  With conf the confidence maps (color_ref.confidence_map), p2v / v2p the pixel <->
vertex maps of the fusion and C_in the R, G, B of every vertex AS HANDED IN, vertex g of sensor j at pixel pj becomes, per channel,

    floor((sum w c + floor(W / 2)) / W),   W = sum w

over its own term (w = conf_j[pj], c = C_in[g]; always) and one term per other sensor i, in ascending i, for which
(x, y, d1) = project(sensor i, X, Y, Z) (color_ref.project: float32, x64 conversions) gives 0 <= x < w_i, 0 <= y < h_i, d1 != 0,
d2 = depth_i[y, x] > 0, |d1 - d2| < depth_tol, v = p2v_i[y, x] >= 0 and w = conf_i[y, x] >= min_confidence (c = C_in[v]).
A vertex without a partner keeps its bytes; alpha, X, Y, Z never change.  depth_tol <= 0 or min_confidence > 20: off; min_confidence < 1
is read as 1; one sensor: nothing to do; more than 32 sensors: refused.

tests/color_blend_ref_py.py restates it in plain Python loops (and computes the neighbouring wrong rules); tests/color_blend_cases.py
holds the hand-made rigs."""
import numpy as np

from tests import color_ref

MAX_MAPS = 32
CONF_LIMIT = color_ref.ET_LIMIT


class Refused(ValueError):
    pass


def sensors_of(rig, orc):
    """[color_ref.Sensor] of a rig: vertices, pixel <-> vertex maps and confidence map of every sensor."""
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2")
    dc = np.ascontiguousarray(rig.depth_colors)
    out, po = [], 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        out.append(color_ref.Sensor(dm[po:po + w * h].reshape(h, w), dc[3 * po:3 * (po + w * h)].reshape(h, w, 3), rig.intr[7 * s:7 * s + 7],
                                    rig.wt[12 * s:12 * s + 12], rig.bounds, orc))
        po += w * h
    return out


def fused(sensors):
    """The merged cloud as the fusion writes it, and its offsets [n + 1]."""
    off = np.concatenate([[0], np.cumsum([len(s.verts) for s in sensors])]).astype(np.int64)
    return np.concatenate([s.verts for s in sensors]), off


def empty_diag(n):
    return {"blended": np.zeros(n, np.int32), "partners": np.zeros(n, np.int64), "abs_change": np.zeros(n, np.int64)}


def blend(rig, orc, depth_tol, min_confidence, verts=None, sensors=None, terms=None):
    """-> (vertices VERTEX_DTYPE, {"blended": int32[n], "partners": int64[n], "abs_change": int64[n]}).
    verts: the cloud to blend (default: as fused); terms: an optional list that receives, per (j, i != j), a dict of what every vertex of j
    met in sensor i (x, y, d1, d2, w, v, inside, took_part and the numerator / weight sums are in "sums" of the (j, None) entry): what
    the cases' witnesses read."""
    S = sensors_of(rig, orc) if sensors is None else sensors
    n = len(S)
    if n > MAX_MAPS:
        raise Refused(f"at most {MAX_MAPS} sensors (the rig has {n})")
    base, off = fused(S)
    cur = base.copy() if verts is None else np.array(verts, dtype=base.dtype, copy=True)
    assert len(cur) == off[-1]
    diag = empty_diag(n)
    if depth_tol <= 0 or min_confidence > CONF_LIMIT or n == 1:
        return cur, diag
    mc = max(int(min_confidence), 1)
    C = np.stack([cur["R"], cur["G"], cur["B"]], axis=1).astype(np.int64)      # C_in: never written below
    out = C.copy()
    for j, sj in enumerate(S):
        g0, g1 = int(off[j]), int(off[j + 1])
        W = sj.conf[sj.v2p].astype(np.int64)
        num = W[:, None] * C[g0:g1]
        k = np.zeros(g1 - g0, np.int64)
        for i, si in enumerate(S):
            if i == j:
                continue
            x, y, d1 = color_ref.project(cur["X"][g0:g1], cur["Y"][g0:g1], cur["Z"][g0:g1], si.intr, si.wt)
            inside = (x >= 0) & (x < si.w) & (y >= 0) & (y < si.h)
            q = np.where(inside, x + y * si.w, 0)
            d2 = si.depth.ravel()[q].astype(np.int64)
            w = si.conf[q].astype(np.int64)
            v = si.p2v[q].astype(np.int64)
            ok = inside & (d1 != 0) & (d2 > 0) & (np.abs(d1 - d2) < depth_tol) & (v >= 0) & (w >= mc)
            W = W + np.where(ok, w, 0)
            num = num + np.where(ok[:, None], w[:, None] * C[np.where(ok, off[i] + v, 0)], 0)
            k += ok
            if terms is not None:
                terms.append(dict(j=j, i=i, x=x, y=y, d1=d1, d2=d2, w=w, v=v, inside=inside, took_part=ok))
        has = k > 0
        assert (W >= 1).all() and int(num.max(initial=0)) <= MAX_MAPS * CONF_LIMIT * 255
        new = (num + (W // 2)[:, None]) // W[:, None]
        out[g0:g1][has] = new[has]
        diag["blended"][j] = int(has.sum())
        diag["partners"][j] = int(k.sum())
        diag["abs_change"][j] = int(np.abs(out[g0:g1] - C[g0:g1]).sum())
        if terms is not None:
            terms.append(dict(j=j, i=None, W=W, num=num, has=has, own=sj.conf[sj.v2p].astype(np.int64)))
    cur["R"], cur["G"], cur["B"] = out[:, 0].astype(np.uint8), out[:, 1].astype(np.uint8), out[:, 2].astype(np.uint8)
    return cur, diag
