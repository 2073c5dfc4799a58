"""CPU reference of generateMeshFromDepthMaps' colour transfer (bcolor_transfer = true).  TEST INFRASTRUCTURE ONLY.

A line-cited restatement (numpy) of the reference's stages, on top of the CPU oracle's vertex generation (oracle/orc.py
create_vertices: createVertices, depthprocessing.cpp:122-186):

  1. confidence       generateMapConfidence            src/NativeUtils/depthprocessing.cpp:285-384 (et_limit 20, threshold 20, :390-393)
  2. coverage         calculateMapsCoverage            :1387-1424, pointProjection :735-747, WorldTranformation::inv depthprocessing.h:65-75
  3. pairing          updateColorCorrectionCoefficients :1491-1561
  4. transform        getColorCorrectionTransform      :1426-1489, colorcorrection.cpp:6-96 (CS_RGB)
  5. apply            applyColorCorrection             :1563-1575, colorcorrection.cpp:139-170

and the two places where the behaviour is defined rather than copied:
  * a transform sample whose pixel in the base sensor i has depth but no vertex (depth_to_vertices_map == -1, :1457) is skipped
    (the reference reads colors1[-3..-1]); the coverage counts it, as the reference does;
  * (int) of a double that is NaN or out of range gives INT_MIN (x64 cvttsd2si), so the clamp gives 0.

tests/color_ref_py.py restates steps 1-5 again in plain Python loops; tests/golden/color_transfer_ref.npz pins steps 4-5 to the
reference's own colorcorrection.cpp (tests/golden/make_color_golden.py), and tests/golden/export_ref.npz / export_ref_digests.json
pin steps 1-5 together to the reference's own generateMeshFromDepthMaps(bcolor_transfer = true) (tests/golden/make_export_golden.py,
tests/test_export_pin.py).  The first defined place above (a crop box through the overlap) is not in those fixtures: there the
reference reads out of bounds, so this restatement is the definition."""
import numpy as np

ET_LIMIT = 20          # :392
DEPTH_THRESHOLD = 20   # :393, :1401, :1442
MIN_CONFIDENCE = 5     # :1412, :1461
COVERAGE_THRESHOLD = 100  # :1498
INT_MIN = -2 ** 31


def cvt_i32_x64(v):
    """(int)v of float64 values as x64 code computes it: truncation, INT_MIN for NaN and anything outside int32 after truncation."""
    v = np.asarray(v, dtype=np.float64)
    ok = (v > -2147483649.0) & (v < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, v, 0.0)), INT_MIN).astype(np.int64)


def confidence_map(depth):
    """generateMapConfidence (:285-384) on one sensor's full depth map (h, w) u16 -> (h, w) u8."""
    d = np.asarray(depth).astype(np.int64)
    h, w = d.shape
    conf = np.full((h, w), ET_LIMIT, dtype=np.int64)     # :291
    if w < 3 or h < 3:
        return conf.astype(np.uint8)
    inner = np.zeros((h, w), dtype=bool)
    inner[1:h - 1, 1:w - 1] = True
    conf[inner & (d == 0)] = 0                             # :310-314
    # the wall test probes (x + shift_x, y + shift_x) (:320: shift_x in the row offset too) = (-1,-1), (0,0), (1,1)
    c = d[1:h - 1, 1:w - 1]
    nw, se = d[0:h - 2, 0:w - 2], d[2:h, 2:w]
    wall = (np.abs(c - nw) > DEPTH_THRESHOLD) | (nw == 0) | (np.abs(c - se) > DEPTH_THRESHOLD) | (se == 0)
    seed = np.zeros((h, w), dtype=bool)
    seed[1:h - 1, 1:w - 1] = wall & (c != 0)
    conf[seed] = 1                                         # :328-334
    frontier = seed
    level = 1                                              # max_et (:339)
    ys, xs = np.mgrid[0:h, 0:w]
    visitable = (xs > 0) & (ys > 0) & (d != 0)             # :356-357 (x == w-1 / y == h-1 stay visitable), :361
    pad = lambda a, fill: np.pad(a, 1, constant_values=fill)
    while frontier.any() and level != ET_LIMIT:            # :339
        fp, dp = pad(frontier, False), pad(d, 0)
        new = np.zeros((h, w), dtype=bool)
        cand = visitable & (conf == ET_LIMIT)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                # a frontier pixel at (x - dx, y - dy) reaches (x, y)
                f_n = fp[1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
                d_n = dp[1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
                new |= cand & f_n & (np.abs(d_n - d) < DEPTH_THRESHOLD)
        conf[new] = level + 1                              # :364
        frontier = new
        level += 1
    return conf.astype(np.uint8)


def _inverse(wt12):
    """WorldTranformation(float*) (depthprocessing.h:56-63: t = wt[0:3], R = wt[3:12] row-major) then inv(): R^T and -t."""
    wt12 = np.asarray(wt12, dtype=np.float32)
    return wt12[3:12].reshape(3, 3).T.copy(), -wt12[0:3]


def project(X, Y, Z, intr7, wt12):
    """pointProjection (:735-747) into the sensor of intr7 / wt12 with its inverted transform: float32 arithmetic in the reference's
    order, the + 0.5 in double, the int conversions as x64 does them.  Returns (x, y, d) int64 arrays."""
    R, t = _inverse(wt12)
    f32 = np.float32
    X, Y, Z = (np.asarray(a, dtype=f32) for a in (X, Y, Z))
    tx = X * R[0, 0] + Y * R[0, 1] + Z * R[0, 2]           # RotatePoint (:109-120)
    ty = X * R[1, 0] + Y * R[1, 1] + Z * R[1, 2]
    tz = X * R[2, 0] + Y * R[2, 1] + Z * R[2, 2]
    tx, ty, tz = tx + t[0], ty + t[1], tz + t[2]
    cx, cy, fx, fy = (f32(v) for v in np.asarray(intr7, dtype=f32)[:4])   # IntrinsicCameraParameters(float*), depthprocessing.h:96-97
    with np.errstate(all="ignore"):
        x = cvt_i32_x64(((tx * fx) / tz + cx).astype(np.float64) + 0.5)
        y = cvt_i32_x64((cy - (ty * fy) / tz).astype(np.float64) + 0.5)
        d = np.clip(cvt_i32_x64((tz * f32(1000.0)).astype(np.float64)), 0, 65535)
    return x, y, d


class Sensor:
    def __init__(self, depth, rgb, intr7, wt12, bounds, orc):
        self.depth = np.ascontiguousarray(depth, dtype=np.uint16)
        self.h, self.w = self.depth.shape
        self.intr, self.wt = np.asarray(intr7, np.float32), np.asarray(wt12, np.float32)
        self.verts, self.v2p, self.p2v = orc.create_vertices(depth, rgb, intr7, wt12, bounds, want_maps=True)
        self.conf = confidence_map(self.depth).ravel()
        self.colors = np.stack([self.verts["R"], self.verts["G"], self.verts["B"]], axis=1).astype(np.int64)


def _tests(si, sj, with_d1):
    """The per-vertex tests of calculateMapsCoverage (with_d1) / getColorCorrectionTransform on the vertices of sj projected into si.
    Returns (mask over sj's vertices, the projected pixel index into si)."""
    x, y, d1 = project(sj.verts["X"], sj.verts["Y"], sj.verts["Z"], si.intr, si.wt)
    inb = (x >= 0) & (x < si.w) & (y >= 0) & (y < si.h)
    if with_d1:
        inb &= d1 != 0
    q = np.where(inb, x + y * si.w, 0)
    ok = inb & (si.conf[q] >= MIN_CONFIDENCE) & (sj.conf[sj.v2p] >= MIN_CONFIDENCE)
    d2 = si.depth.ravel()[q].astype(np.int64)
    ok &= (d2 > 0) & (np.abs(d1 - d2) < DEPTH_THRESHOLD)
    return ok, q


def coverage(si, sj):
    ok, _ = _tests(si, sj, True)
    return int(ok.sum())


def choose_pairs(cov):
    """updateColorCorrectionCoefficients' greedy loop (:1507-1560) on the symmetric table."""
    n = len(cov)
    assigned = [False] * n
    pairs = []
    while True:
        best, b1, b2 = 0, None, None
        for i in range(n):
            for j in range(n):
                if i == j or assigned[j] or not assigned[i]:
                    continue
                if cov[i][j] > best:
                    best, b1, b2 = cov[i][j], i, j
        if best == 0:
            for i in range(n):
                for j in range(i + 1, n):
                    if cov[i][j] > best and not assigned[i] and not assigned[j]:
                        best, b1, b2 = cov[i][j], i, j
        if best <= COVERAGE_THRESHOLD:
            return pairs
        assigned[b1] = assigned[b2] = True
        pairs.append((b1, b2))


def transform(src, dst):
    """getColorCorrectionTransform(RGB_source, RGB_dst, CS_RGB) (colorcorrection.cpp:6-96) on (n, 3) integer samples.
    Returns 9 float64: mean_src[3], mean_dst[3], scale[3].  Empty: means 0, scales 1 (the early return, :10-11; RGB by definition)."""
    src, dst = np.asarray(src, np.int64).reshape(-1, 3), np.asarray(dst, np.int64).reshape(-1, 3)
    n = len(src)
    if n == 0:
        return np.array([0.0] * 6 + [1.0] * 3)
    m1 = src.sum(axis=0).astype(np.float64) / max(1.0, float(n))       # :53-62 (integer sums: exact)
    m2 = dst.sum(axis=0).astype(np.float64) / max(1.0, float(n))
    # :64-80: sequential double sums (np.add.accumulate folds left to right; np.sum would pair)
    s1 = np.add.accumulate(np.abs(src.astype(np.float64) - m1), axis=0)[-1] / float(n) + 1e-15
    s2 = np.add.accumulate(np.abs(dst.astype(np.float64) - m2), axis=0)[-1] / float(n) + 1e-15
    return np.concatenate([m1, m2, s1 / s2])


def apply(rgb, xf):
    """applyColorCorrection (colorcorrection.cpp:139-170, CS_RGB) on (m, 3) bytes -> (m, 3) uint8."""
    c = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    v = (c - xf[3:6]) * xf[6:9] + xf[0:3]
    return np.clip(cvt_i32_x64(v), 0, 255).astype(np.uint8)


def color_transfer(rig, orc):
    """The merged cloud of generateMeshFromDepthMaps(bcolor_transfer = true) for a synth.Rig, with what led to it.
    Returns (vertices VERTEX_DTYPE, {"confidence": u8 per tick pixel, "coverage": (n, n), "pairs": [...], "transforms": (k, 9)})."""
    sensors = []
    dm = np.ascontiguousarray(rig.depth_maps).view("<u2")
    dc = np.ascontiguousarray(rig.depth_colors)
    po = co = 0
    for s in range(rig.n):
        w, h = int(rig.widths[s]), int(rig.heights[s])
        sensors.append(Sensor(dm[po:po + w * h].reshape(h, w), dc[co:co + 3 * w * h].reshape(h, w, 3), rig.intr[7 * s:7 * s + 7],
                              rig.wt[12 * s:12 * s + 12], rig.bounds, orc))
        po += w * h
        co += 3 * w * h
    n = rig.n
    cov = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(i + 1, n):
            cov[i, j] = cov[j, i] = coverage(sensors[i], sensors[j])
    pairs = choose_pairs(cov.tolist())
    xfs = []
    for i, j in pairs:   # all from the uncorrected colours (:1545 before :1763)
        si, sj = sensors[i], sensors[j]
        ok, q = _tests(si, sj, False)
        gi = si.p2v[q]
        ok &= gi >= 0    # defined: no vertex of i at the pixel -> no sample
        xfs.append(transform(si.colors[gi[ok]], sj.colors[ok]))
    out = [s.verts.copy() for s in sensors]
    for (i, j), xf in zip(pairs, xfs):
        c = apply(sensors[j].colors, xf)
        out[j]["R"], out[j]["G"], out[j]["B"] = c[:, 0], c[:, 1], c[:, 2]
    verts = np.concatenate(out) if out else np.zeros(0, dtype=sensors[0].verts.dtype)
    diag = {"confidence": np.concatenate([s.conf for s in sensors]), "coverage": cov, "pairs": pairs,
            "transforms": np.array(xfs).reshape(-1, 9)}
    return verts, diag
