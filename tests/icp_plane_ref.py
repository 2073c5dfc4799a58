"""One point-to-plane ICP iteration after the neighbour search, as a plain definition -- numpy only.

The stage is DEFINED here, not copied: the reference has point-to-point ICP only (tests/icp_step_ref.py).  `step` states in
float64 what one iteration computes from the exact nearest-neighbour result, the target's points and normals and the source:

  1. matching, statistics, rejection: exactly icp_step_ref.step's (one-to-one winners, the later query wins ties, f32-style mean
     and sigma, keep iff !(d2 > 2.5 sigma)); m, mean, sd mean what they mean there.
  2. usable matches: a kept match whose target normal n (f32, at the target's original index) is finite in all three
     components and has (nx nx + ny ny) + nz nz > 0 evaluated in f32.  Normals are used as given, never renormalised.  mk counts
     the usable matches.
  3. per usable match, in double from the f32 inputs, in THIS operation order (one rounding per operation, no contraction):
         d = b - a                      r  = (d0 n0 + d1 n1) + d2 n2
         J = [b x n, n]                 b x n = (b1 n2 - b2 n1, b2 n0 - b0 n2, b0 n1 - b1 n0)
     (a product of two f32 values is exact in double, so every term J_i J_j, J_i r has a fixed value: an implementation in IEEE
     double reproduces each TERM bit for bit and can differ in the order of the SUMS only).  A = sum J J^T (21 distinct sums),
     g = sum J r (6 sums); the definition takes the exactly rounded sums (math.fsum).
  4. A x = -g by pseudo-inverse over A's eigen-decomposition: an eigenvalue lambda <= CUTOFF lambda_max is unconstrained and
     gets zero step.  CUTOFF = 2^-20 is part of the definition, not a tolerance: the inputs are f32, whose rounding already
     perturbs A's eigenvalues by about 2 2^-24 lambda_max in absolute terms, so anything below 2^-20 lambda_max is
     indistinguishable from zero.  mk == 0 or lambda_max == 0: no motion (T = 0, Rn = I), as in the point-to-point step.
  5. x = (omega, tau); Rinc = exp([omega]x) = I + s K + c K^2 (Rodrigues, double) with s = sin th / th, c = (1 - cos th) / th^2
     and, below th = SERIES_BELOW = 2^-10, their series to th^6 (the next terms are < 2^-80 / 9! there); omega == 0 gives exactly
     I.  The library moves row vectors by v' = (v + T) Rn, so Rn = Rinc^T and T = Rinc^T tau, each rounded once to f32.
  6. apply and pose update: icp_step_ref.apply32 / compose32, bit for bit.

`bounds` derives the tolerances a device implementation that sums in double is held to, from the definition's own quantities."""
import math

import numpy as np

from tests.icp_step_ref import EPS32, EPS64, F32, apply32, compose32, ulp32, winners  # noqa: F401  (apply32 / compose32: part of this definition)

CUTOFF = 2.0 ** -20
SERIES_BELOW = 2.0 ** -10
TRI = [(i, j) for i in range(6) for j in range(i, 6)]      # the 21 distinct sums of A, row-major upper triangle


def match(idx, d2):
    """Step 1, exactly as icp_step_ref.step states it."""
    idx = np.asarray(idx, dtype=np.int64)
    d2 = np.asarray(d2, dtype=F32)
    w = winners(idx, d2)
    d = d2[w].astype(np.float64)
    m = len(w)
    mean = d.sum() / m
    dev2 = ((d - mean) ** 2).sum()
    sd = np.sqrt(dev2 / m)
    thresh = 2.5 * sd
    keep = ~(d > thresh)
    margin = float(np.abs(d - thresh).min() / thresh) if thresh > 0 else np.inf
    return dict(winners=w, m=m, mean=mean, sd=sd, thresh=thresh, keep=keep, kept=w[keep], margin=margin, sum_d2=float((d * d).sum()),
                dev2=float(dev2))


def usable(nrm32):
    """Step 2 on an [k, 3] f32 array of normals."""
    n = np.asarray(nrm32, dtype=F32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return np.isfinite(n).all(axis=1) & (nn > 0)


def terms(a, n, b):
    """Step 3 per match: (J [k, 6], r [k]) in double from f32 inputs, in the stated operation order."""
    a, n, b = (np.asarray(v, dtype=F32).reshape(-1, 3).astype(np.float64) for v in (a, n, b))
    d = b - a
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = np.empty((len(a), 6))
    J[:, 0] = b[:, 1] * n[:, 2] - b[:, 2] * n[:, 1]
    J[:, 1] = b[:, 2] * n[:, 0] - b[:, 0] * n[:, 2]
    J[:, 2] = b[:, 0] * n[:, 1] - b[:, 1] * n[:, 0]
    J[:, 3:] = n
    return J, r


def normal_equations(J, r):
    """A, g as exactly rounded sums, and the elementwise absolute sums sum |J J^T|, sum |J r| the bounds need."""
    A, absA = np.zeros((6, 6)), np.zeros((6, 6))
    for i, j in TRI:
        p = J[:, i] * J[:, j]
        A[i, j] = A[j, i] = math.fsum(p)
        absA[i, j] = absA[j, i] = math.fsum(np.abs(p))
    q = J * r[:, None]
    g = np.array([math.fsum(q[:, i]) for i in range(6)])
    absg = np.array([math.fsum(np.abs(q[:, i])) for i in range(6)])
    return A, g, absA, absg


def solve(A, g, cutoff=CUTOFF, sign=-1.0):
    """Step 4.  Returns (x, eigenvalues ascending, eigenvectors as columns, kept mask)."""
    lam, V = np.linalg.eigh(A)
    lam_max = lam.max()
    if not lam_max > 0:
        return np.zeros(6), lam, V, np.zeros(6, bool)
    kept = lam > cutoff * lam_max
    c = V.T @ g
    x = sign * (V[:, kept] @ (c[kept] / lam[kept]))
    return x, lam, V, kept


def rodrigues(w):
    """exp([w]x) in double; exactly I for w == 0."""
    w = np.asarray(w, dtype=np.float64)
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(t2)
    if th < SERIES_BELOW:
        s = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0 * (1.0 - t2 / 42.0))
        c = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0 * (1.0 - t2 / 56.0))
    else:
        s = np.sin(th) / th
        c = (1.0 - np.cos(th)) / t2
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return np.eye(3) + s * K + c * (K @ K)


def motion(x, rn_transposed=True, t_rotated=True):
    """Step 5: (T, Rn) in double, before their one rounding to f32.  The two flags are the WRONG forms the mutant tests need."""
    Rinc = rodrigues(x[:3])
    Rn = Rinc.T if rn_transposed else Rinc
    T = Rinc.T @ x[3:] if t_rotated else np.array(x[3:], dtype=np.float64)
    return T, Rn


def step(tgt, nrm, src, idx, d2, cutoff=CUTOFF, g_sign=-1.0, cross_of="b", rn_transposed=True, t_rotated=True):
    """One iteration in float64 from the exact NN result.  The keyword arguments select WRONG variants of the definition (the
    mutants tests/test_icp_plane_ref.py kills); the defaults are the definition."""
    tgt32 = np.asarray(tgt, dtype=F32).reshape(-1, 3)
    nrm32 = np.asarray(nrm, dtype=F32).reshape(-1, 3)
    src32 = np.asarray(src, dtype=F32).reshape(-1, 3)
    idx = np.asarray(idx, dtype=np.int64)
    out = match(idx, d2)
    wk = out["kept"]
    use = usable(nrm32[idx[wk]])
    wu = wk[use]
    mk = len(wu)
    out.update(n_kept=len(wk), used=wu, mk=mk)
    none = dict(A=np.zeros((6, 6)), g=np.zeros(6), absA=np.zeros((6, 6)), absg=np.zeros(6), x=np.zeros(6), lam=np.zeros(6), V=np.eye(6),
                kept_modes=np.zeros(6, bool), T=np.zeros(3), Rn=np.eye(3))
    if mk == 0:
        out.update(none)
        return out
    a, n, b = tgt32[idx[wu]], nrm32[idx[wu]], src32[wu]
    J, r = terms(a, n, b)
    if cross_of == "a":
        J[:, :3] = terms(a, n, a)[0][:, :3]
    A, g, absA, absg = normal_equations(J, r)
    x, lam, V, kept_modes = solve(A, g, cutoff, g_sign)
    if not kept_modes.any():
        out.update(none)
        out.update(A=A, g=g, absA=absA, absg=absg, lam=lam, V=V)
        return out
    T, Rn = motion(x, rn_transposed, t_rotated)
    out.update(A=A, g=g, absA=absA, absg=absg, x=x, lam=lam, V=V, kept_modes=kept_modes, T=T, Rn=Rn, J=J, r=r)
    return out


def bounds(s):
    """Tolerances (absolute, elementwise) for T and Rn of an implementation that forms the terms as stated, sums them in double in any
    order without atomics, solves in double and rounds T and Rn once to f32.  Everything comes from the definition's own quantities.

    Sums.   Every term is reproduced exactly (see the module docstring); the definition's sums are exactly rounded; a sum of mk terms
            in any order makes at most mk - 1 inexact additions (adding an exact zero is exact), each off by at most 2^-53 of a partial
            sum that never exceeds the absolute sum.  So |dA| <= mk 2^-53 sum |J J^T| and |dg| <= mk 2^-53 sum |J r| elementwise; the
            norms below are Frobenius / Euclidean norms of those.
    Eigen.  Both eigen-solvers (LAPACK here, cyclic Jacobi on the device) are backward stable: each returns the exact
            decomposition of a matrix within p(6) 2^-53 lambda_max of its input with a modest p; 64 2^-53 lambda_max covers both and is
            added to |dA|.
    Solve.  Inside the kept subspace x solves A_k x = -g_k with lambda_min(A_k) = lambda_kept,min:
                |dx|_1 <= (|dA| |x| + |dg|) / (lambda_kept,min - |dA|)                              (linear-solve perturbation)
    Subspace.  The kept invariant subspace turns by at most phi = |dA| / (lambda_kept,min - lambda_dropped,max - |dA|) (Davis-Kahan;
            zero when no mode is dropped).  A turn by phi moves x by at most phi |x| for each of the two projections in
            x = -P A^+ P g and lets at most phi |g| of g into the kept directions, where it is divided by at least lambda_kept,min:
                |dx|_2 <= phi (2 |x| + |g| / lambda_kept,min)
            The regime conditions of the cases (every lambda / lambda_max below 2^-40 or above 2^-10) keep both arithmetics on the same
            side of the cutoff, and the gap at least (2^-10 - 2^-40) lambda_max.
    Motion. Rn = exp(-[omega]x) is 1-Lipschitz in omega (|dRn|_2 <= |d omega|) and T = Rinc^T tau gives |dT| <= |d tau| + |tau| |d omega|;
            both with |d omega|, |d tau| <= |dx| = |dx|_1 + |dx|_2.  Evaluating Rodrigues and the 3x3 products in double on either side
            costs at most 32 2^-53 (1 + |tau|).  The one rounding to f32 of a value within delta of y lands within delta + ulp32(y) of y
            (half an ulp of the rounded value, which may sit one binade above y).
    Returns {"T": [3], "Rn": [3, 3], "dx": float}; all zero when mk == 0 or no mode is kept (then T = 0 and Rn = I exactly)."""
    if s["mk"] == 0 or not s["kept_modes"].any():
        return {"T": np.zeros(3), "Rn": np.zeros((3, 3)), "dx": 0.0}
    lam, kept = s["lam"], s["kept_modes"]
    lam_max, lam_kmin = lam.max(), lam[kept].min()
    dA = s["mk"] * EPS64 * np.linalg.norm(s["absA"]) + 64 * EPS64 * lam_max
    dg = s["mk"] * EPS64 * np.linalg.norm(s["absg"])
    xn, gn = np.linalg.norm(s["x"]), np.linalg.norm(s["g"])
    dx = (dA * xn + dg) / (lam_kmin - dA)
    if not kept.all():
        gap = lam_kmin - max(lam[~kept].max(), 0.0) - dA
        dx += dA / gap * (2 * xn + gn / lam_kmin)
    tau = np.linalg.norm(s["x"][3:])
    ev = 32 * EPS64 * (1 + tau)
    return {"T": dx * (1 + tau) + ev + ulp32(s["T"]), "Rn": dx + ev + ulp32(s["Rn"]), "dx": float(dx)}
