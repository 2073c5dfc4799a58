"""Pure-Python restatement of MeshGenerator::generateTrianglesGradients (src/NativeUtils/meshGenerator.cpp:14-181), including the
4-thread row-band split the reference uses (:147-181), and an instrumented copy of it that reports what every evaluated triangle saw.
TEST INFRASTRUCTURE ONLY: no torch, no native library; shared by tests/test_oracle_triangles.py, tests/tri_cases.py and the boundary
tests."""
import numpy as np

# The corners of a pixel's stencil as (dx, dy): P, U = up, UR = up-right, R = right.
P, U, UR, R = (0, 0), (0, -1), (1, -1), (1, 0)
# The corners checkTriangleConstraints is called with for candidate triangle i, in call order (:117-123): edge j runs from corner j to
# corner (j + 1) % 3.
CHECK_CORNERS = ((P, U, R), (R, U, UR), (P, U, UR), (P, UR, R))
# The corners triangle i is emitted with (triangles_shifts, :101-104).
EMIT_CORNERS = ((R, U, P), (R, UR, U), (P, UR, U), (P, R, UR))
RULES = ("abs", "fwd", "bwd")


def threshold(v0, v1, v2):
    return int((v0 + v1 + v2) / 3.0 * 0.00272 + 7.273)                  # :26, in double


def py_check(depth, p1, p2, p3):
    vals = [int(depth[p1]), int(depth[p2]), int(depth[p3])]
    ptrs = [p1, p2, p3]
    if 0 in vals:
        return False
    thr = int((vals[0] + vals[1] + vals[2]) / 3.0 * 0.00272 + 7.273)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        v1, v2 = vals[a], vals[b]
        if abs(v1 - v2) < thr:
            continue
        shift = ptrs[b] - ptrs[a]
        vf = int(depth[ptrs[b] + shift])
        if vf != 0 and abs(v2 - v1 - (vf - v2)) < thr:
            continue
        vb = int(depth[ptrs[a] - shift])
        if vb != 0 and abs(v2 - v1 - (v1 - vb)) < thr:
            continue
        return False
    return True


def py_region(depth, p2v, w, h, min_y, max_y, out):
    min_x, max_x = 1, w - 2
    min_y, max_y = max(min_y, 2), min(max_y, h - 2)
    up, upright, right = -w, -w + 1, 1
    tshift = [(right, up, 0), (right, upright, up), (0, upright, up), (0, right, upright)]
    for y in range(min_y, max_y):
        for x in range(min_x, max_x):
            p = y * w + x
            if p2v[p] == -1:
                continue
            tr = [py_check(depth, p, p + up, p + right), py_check(depth, p + right, p + up, p + upright), False, False]
            if not tr[0] and not tr[1]:
                tr[2] = py_check(depth, p, p + up, p + upright)
                tr[3] = py_check(depth, p, p + upright, p + right)
            for i in range(4):
                if tr[i]:
                    m = [int(p2v[p + s]) for s in tshift[i]]
                    if -1 not in m:
                        out.append(m)


def py_triangles(depth2d, p2v):
    h, w = depth2d.shape
    depth = depth2d.ravel()
    out = []
    step, pos = h // 4 + 1, 0                       # generateTrianglesGradients :147-181: 4 bands, concatenated in order
    for _ in range(4):
        size = min(step, h - pos)
        py_region(depth, p2v, w, h, pos, pos + size, out)
        pos += size
    return np.array(out, dtype=np.int32).reshape(-1, 3)


# ---- the instrumented copy ---------------------------------------------------------------------------------------------------------

def trace_triangle(depth2d, x, y, i):
    """What checkTriangleConstraints sees for candidate triangle i of pixel (x, y), with NO short cut: every edge's three differences
    are computed whether or not an earlier one decided.  Returns None when a corner is 0 (:22-23), else a dict with
      thr      the triangle's threshold,
      edges    three dicts {"abs", "fwd", "bwd"}: the difference each rule compares with thr (None: the rule's probe is 0, it cannot pass),
      verdict  what checkTriangleConstraints returns."""
    c = CHECK_CORNERS[i]
    v = [int(depth2d[y + dy, x + dx]) for dx, dy in c]
    if 0 in v:
        return None
    thr = threshold(*v)
    edges = []
    for j in range(3):
        (ax, ay), (bx, by) = c[j], c[(j + 1) % 3]
        v1, v2 = v[j], v[(j + 1) % 3]
        sx, sy = bx - ax, by - ay
        vf = int(depth2d[y + by + sy, x + bx + sx])
        vb = int(depth2d[y + ay - sy, x + ax - sx])
        edges.append({"abs": abs(v1 - v2),
                      "fwd": abs(v2 - v1 - (vf - v2)) if vf != 0 else None,
                      "bwd": abs(v2 - v1 - (v1 - vb)) if vb != 0 else None})
    verdict = all(any(e[r] is not None and e[r] < thr for r in RULES) for e in edges)
    return {"thr": thr, "edges": edges, "verdict": verdict}


def trace_pixel(depth2d, p2v, x, y):
    """The reference's treatment of pixel (x, y), 1 <= x < w - 2, 2 <= y < h - 2.  Returns a dict with
      skipped    the pixel has no vertex (:113-114): nothing is evaluated,
      traces     trace_triangle of triangles 0 .. 3; 2 and 3 are None ("not evaluated") unless neither 0 nor 1 passed (:120),
      verdicts   the four verdicts (a triangle that was not evaluated: False),
      emitted    the triangles that are emitted: a true verdict whose three vertex indices exist (:133-134)."""
    h, w = depth2d.shape
    assert 1 <= x < w - 2 and 2 <= y < h - 2
    if p2v[y * w + x] == -1:
        return {"skipped": True, "traces": [None] * 4, "verdicts": [False] * 4, "emitted": []}
    traces = [trace_triangle(depth2d, x, y, 0), trace_triangle(depth2d, x, y, 1), None, None]
    verdicts = [bool(t and t["verdict"]) for t in traces]
    if not verdicts[0] and not verdicts[1]:
        for i in (2, 3):
            traces[i] = trace_triangle(depth2d, x, y, i)
            verdicts[i] = bool(traces[i] and traces[i]["verdict"])
    emitted = [i for i in range(4) if verdicts[i] and all(p2v[(y + dy) * w + x + dx] != -1 for dx, dy in EMIT_CORNERS[i])]
    return {"skipped": False, "traces": traces, "verdicts": verdicts, "emitted": emitted}


def pixel_triangles(p2v, w, x, y, emitted):
    """The index triples pixel (x, y) emits for the triangle numbers `emitted`."""
    return [[int(p2v[(y + dy) * w + x + dx]) for dx, dy in EMIT_CORNERS[i]] for i in emitted]
