"""One ICP iteration after the neighbour search (icp.cpp:95-168), as a plain definition -- numpy only.

`step` states in float64 what one iteration computes from the exact nearest-neighbour result: the one-to-one matching, the
statistics and the 2.5 sigma rejection, the mean difference T, the cross-covariance M and its orthogonal polar factor Rn.
`apply32` and `compose32` state the motion and the pose update in float32 with one rounding per operation, in the operation
order of apply_kernel / solve_kernel (icp.hip), which is the reference's (icp.cpp:143-146, :165-168).  `bounds` derives the
tolerances a float32 / double implementation of the step is held to -- from the definition's own quantities, never from
the output under test.  tests/test_icp_step_ref.py ties this module to the C oracle (oracle/lsn_oracle.c), which carries
icp.cpp's line references; tests/test_icp_step_gpu.py holds the HIP kernels to it."""
import numpy as np

F32 = np.float32
EPS32 = 2.0 ** -24   # unit roundoff of float32
EPS64 = 2.0 ** -53


def ulp32(x):
    """Spacing of float32 at |x| (elementwise)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def winners(idx, d2):
    """The one-to-one matching (icp.cpp:95-126): per target the query with the smallest f32 distance; among equal distances
    the LARGEST query index (the sequential scan lets a later query replace an earlier one unless it is strictly farther,
    icp.cpp:103).  Returns the winning query indices in ascending order."""
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=F32)
    i = np.arange(len(idx), dtype=np.int64)
    order = np.lexsort((-i, d2, idx))                      # by target, then distance, then query index descending
    first = np.ones(len(order), bool)
    first[1:] = idx[order][1:] != idx[order][:-1]
    return np.sort(order[first])


def step(tgt, src, idx, d2, tie="last"):
    """One iteration in float64 from the exact NN result (idx[i], d2[i] = the f32 squared distance of query i's neighbour).
    tie="first" is the WRONG tie rule (lowest query index wins), kept for the case builders that must show a case depends on it."""
    tgt64 = np.asarray(tgt, dtype=np.float64).reshape(-1, 3)
    src64 = np.asarray(src, dtype=np.float64).reshape(-1, 3)
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=F32)
    if tie == "last":
        w = winners(idx, d2)
    else:
        n = len(idx)
        w = n - 1 - winners(idx[::-1], d2[::-1])[::-1]
    d = d2[w].astype(np.float64)
    m = len(w)
    mean = d.sum() / m
    dev2 = ((d - mean) ** 2).sum()
    sd = np.sqrt(dev2 / m)
    thresh = 2.5 * sd
    keep = ~(d > thresh)                                   # icp.cpp:64: only d > thresh is rejected
    if thresh > 0:
        margin = float(np.abs(d - thresh).min() / thresh)
    else:
        margin = np.inf                                    # thresh is exactly 0 in any arithmetic: d > 0 goes, d == 0 stays
    wk = w[keep]
    mk = len(wk)
    out = dict(winners=w, m=m, mean=mean, sd=sd, thresh=thresh, keep=keep, kept=wk, mk=mk, margin=margin,
               sum_d2=float((d * d).sum()), dev2=float(dev2), coord_max=float(max(np.abs(tgt64).max(), np.abs(src64).max())))
    if mk == 0:
        # the reference would throw in cv::reduce on an empty matrix; the project's defined behaviour is "no motion"
        out.update(T=np.zeros(3), M=np.zeros((3, 3)), sigma=np.zeros(3), Rn=np.eye(3), flipped=False, sum_a=np.zeros(3))
        return out
    a = tgt64[idx[wk]]
    b = src64[wk]
    T = (a - b).sum(axis=0) / mk                           # icp.cpp:141
    M = (b + T).T @ a                                      # icp.cpp:152: M = sum (b + T) a^T
    U, s, Vt = np.linalg.svd(M)
    flipped = bool(np.linalg.det(U @ Vt) < 0)
    if flipped:                                            # icp.cpp:157-163
        U = U.copy()
        U[:, 2] = -U[:, 2]
    out.update(T=T, M=M, sigma=s, Rn=U @ Vt, flipped=flipped, sum_a=a.sum(axis=0))
    return out


def apply32(v, T, Rn):
    """(v + T) Rn for row vectors in f32, one rounding per operation, in apply_kernel's association:
    x' = (x r0 + y r3) + z r6, ... (icp.cpp:143-146, :165)."""
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    T = np.asarray(T, dtype=F32).ravel()
    r = np.asarray(Rn, dtype=F32).ravel()
    x, y, z = v[:, 0] + T[0], v[:, 1] + T[1], v[:, 2] + T[2]
    out = np.empty_like(v)
    for c in range(3):
        out[:, c] = (x * r[c] + y * r[3 + c]) + z * r[6 + c]
    return out


def compose32(R, t, T, Rn):
    """The f32 pose update of solve_kernel (icp.cpp:167-168): t += T R^T with the OLD R, then R = R Rn.  Returns (R, t)."""
    R = np.asarray(R, dtype=F32).reshape(3, 3)
    t = np.asarray(t, dtype=F32).ravel()
    T = np.asarray(T, dtype=F32).ravel()
    Rn = np.asarray(Rn, dtype=F32).reshape(3, 3)
    add = (T[0] * R[:, 0] + T[1] * R[:, 1]) + T[2] * R[:, 2]
    t_new = t + add
    R_new = np.empty((3, 3), F32)
    for c in range(3):
        R_new[:, c] = (R[:, 0] * Rn[0, c] + R[:, 1] * Rn[1, c]) + R[:, 2] * Rn[2, c]
    return R_new, t_new


def bounds(s):
    """Tolerances for an implementation that sums in double and rounds to f32 where the reference holds f32 values.

    mean    1 ulp of f32 at the f64 mean: a double sum rounded once.
    sd      4 ulp (the f32 roundings of the sum of squares, the division, the square root and the f32 mean the deviations
            are taken from) plus the cancellation of the one-pass formula sum d^2 - 2 mean sum d + m mean^2, whose three terms
            are of size sum d^2 and carry 2^-53 each with their sums: 8 2^-53 sum d^2 / sum (d - mean)^2, relative.
    T       1 ulp per component, plus 1e-12 max|coordinate|: the double sums of a and b cancel when T is near zero.
    Rn      2 |dM|_F / (sigma2 + sigma3) + 12 2^-24.  The first term is the perturbation bound of the orthogonal polar factor
            (for a proper rotation the gap is sigma2 + sigma3; with the reflection fix it is sigma2 - sigma3) under the f32
            rounding of M and of T, which the reference commits as well: |dM| <= 2^-24 (|M| + |T| (x) |sum a|) elementwise.
            The second term is the f32 rounding of U, V^T (9 elements each at <= 2^-24, three per product element) and of
            their product's two additions and three multiplications."""
    b = {"mean": float(ulp32(s["mean"]))}
    if s["dev2"] > 0:
        b["sd"] = float(4 * ulp32(s["sd"]) + s["sd"] * 8 * EPS64 * s["sum_d2"] / s["dev2"])
    else:
        b["sd"] = 0.0
    b["T"] = ulp32(s["T"]) + 1e-12 * s["coord_max"]
    if s["mk"] > 0:
        dM = EPS32 * (np.abs(s["M"]) + np.outer(np.abs(s["T"]), np.abs(s["sum_a"])))
        sg = s["sigma"]
        gap = (sg[1] - sg[2]) if s["flipped"] else (sg[1] + sg[2])
        b["Rn"] = float(2 * np.linalg.norm(dM) / gap + 12 * EPS32) if gap > 0 else np.inf
    else:
        b["Rn"] = 0.0
    return b
