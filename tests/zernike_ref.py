"""Helpers of the Zernike read-out tests (not a test file): the definitions of include/bmo.h "Zernike read-out" in elementwise numpy (which
makes the per-row doubles proj_h, W_h, u_h, v_h, x_h, y_h, Z_j, D_h), exact sums of those doubles taken as data (Python integers after
scaling every column by a power of two), the header's Cholesky restated in Python floats, and the derived error bounds.

The engine evaluates the same per-row expressions, so it sums the same doubles; what is left to bound is the summation and the solve.
U0, V0, RHO, X_REF, Z_REF and W_MEAN enter as the doubles the call returned (as psf_stats_ref.stat_violations does with CX).

Bounds.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1).  n rows, J terms.

  Gram entry   G_ik = sum_h (proj_h * B_i) * B_k: two roundings per term and at most n - 1 additions in any order (each term passes at
               most n - 1 of them): G^_ik = sum_h proj_h B_i B_k (1 + theta_{n+1}):   |G^_ik - G_ik| <= gamma_{n+1} sum_h proj_h |B_i| |B_k|.
  Coefficients a posteriori.  The restated Cholesky of the returned gram gives L^ and c^ (the engine's c^ must equal it bit for bit).  By
               Higham, Thm 10.4, (G^ + dG2) c^ = b^ exactly with |dG2| <= gamma_{3J+1} |L^| |L^T|.  With the exact G, b of the same
               doubles, G c = b, hence G (c^ - c) = (b^ - b) - ((G^ - G) + dG2) c^ and componentwise
                   |c^ - c| <= |G^-1| (|b^ - b| + (|G^ - G| + gamma_{3J+1} |L^| |L^T|) |c^|),
               G^-1 the exact rational inverse, |G^ - G| and |b^ - b| the actual differences of the returned entries to the exact sums.
  FIT_RMS      E_h = D_h - F_h are doubles the engine and numpy compute alike (E_LO / E_HI check them bit for bit).  V = sum proj_h E_h^2 / S:
               per term e * e (1), proj * (.) (2), n - 1 additions, the division (n + 2); the denominator carries gamma_{n-1}:
               theta_{2n+1}, covered by gamma_{2n+2}:  |V^ - V| <= B_V = gamma_{2n+2} V.  The root moves by at most
               B_V / (sqrt(V) + sqrt(max(0, V - B_V))), never more than sqrt(B_V); the correctly rounded sqrt adds u times its result
               (the form of psf_stats_ref.sum_bounds' W_RMS, without the mean's term: E_h are data here).
  U0, V0       when computed: the form of CX, gamma_{2n} sum proj_h |u_h| / S.   RHO, N_OUT: the numpy expressions, bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

import psf_stats_ref as pr
from spot_ref import gamma, sqrt_fraction

U = Fraction(1, 2 ** 53)
INFO_N = 13
(N, STATUS, S, X_REF, Z_REF, U0, V0, RHO, W_MEAN, FIT_RMS, E_LO, E_HI, N_OUT) = range(INFO_N)


def n_terms(order):
    return (order + 1) * (order + 2) // 2


def terms(order):
    """(n, m) in OSA/ANSI order, j = (n (n + 2) + m) / 2"""
    return [(n, m) for n in range(order + 1) for m in range(-n, n + 1, 2)]


def term_index(n, m):
    return (n * (n + 2) + m) // 2


def radial(n, am):
    """q_0 .. q_K of R_n^am(rho) / rho^am in t = rho^2, from the factorial formula"""
    K, f = (n - am) // 2, math.factorial
    return [(-1) ** (K - s) * f(n - K + s) // (f(K - s) * f((n + am) // 2 - K + s) * f(s)) for s in range(K + 1)]


# ------------------------------------------------------------------------------------------------ the per-row doubles
def basis(x, y, order):
    """Z [J, n] by the header's expressions (elementwise numpy: one rounding per operation, left to right, no contraction)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    t = x * x + y * y
    Cc, Sc = [np.ones_like(x)], [np.zeros_like(x)]
    for k in range(order):
        Cc.append(Cc[k] * x - Sc[k] * y)
        Sc.append(Sc[k] * x + Cc[k] * y)
    Z = []
    for n, m in terms(order):
        q = radial(n, abs(m))
        r = np.full_like(t, float(q[-1]))
        for s in range(len(q) - 2, -1, -1):
            r = r * t + float(q[s])
        A = Cc[m] if m >= 0 else Sc[-m]
        nrm = math.sqrt(float(n + 1)) if m == 0 else math.sqrt(float(2 * (n + 1)))  # correctly rounded
        Z.append(nrm * (r * A))
    return np.array(Z)


def cosines(rows, e1, e2):
    """(u_h, v_h): the direction cosines in the detector frame"""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    a, b = np.asarray(e1, dtype=np.float64), np.asarray(e2, dtype=np.float64)
    return (r[:, 3] * a[0] + r[:, 4] * a[1]) + r[:, 5] * a[2], (r[:, 3] * b[0] + r[:, 4] * b[1]) + r[:, 5] * b[2]


def pupil_xy(u, v, u0, v0, rho):
    with np.errstate(all="ignore"):
        return (u - np.float64(u0)) / np.float64(rho), (v - np.float64(v0)) / np.float64(rho)


def columns(rows, pose, info, order):
    """(proj [n], B [J + 1, n], x, y): the augmented columns Z_0 .. Z_{J-1}, D at the doubles `info` returned."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    origin, e1, e2 = pose
    W = pr.paths(r, pr.ref_point(origin, e1, e2, info[X_REF], info[Z_REF]))
    u, v = cosines(r, e1, e2)
    x, y = pupil_xy(u, v, info[U0], info[V0], info[RHO])
    Z = basis(x, y, order)
    return r[:, 7].copy(), np.vstack([Z, (W - np.float64(info[W_MEAN]))[None, :]]), x, y


def residual(B, coef):
    """E_h = D_h - ((c_0 Z_0 + c_1 Z_1) + ...)"""
    J = len(B) - 1
    c = np.asarray(coef, dtype=np.float64)
    F = c[0] * B[0]
    for j in range(1, J):
        F = F + c[j] * B[j]
    return B[J] - F


# ------------------------------------------------------------------------------------------------ exact sums
def _scaled(a):
    """(ints, e): a_h = ints_h * 2^e exactly"""
    a = np.asarray(a, dtype=np.float64)
    assert np.isfinite(a).all()
    m, e = np.frexp(a)
    mi = [int(v * 2 ** 53) for v in m.tolist()]  # |m| in [0.5, 1): m 2^53 is an integer below 2^53, the product is exact
    e = e.astype(np.int64) - 53
    nz = [k for k, v in enumerate(mi) if v]
    if not nz:
        return [0] * len(mi), 0
    e0 = int(min(e[k] for k in nz))
    return [v << (int(e[k]) - e0) if v else 0 for k, v in enumerate(mi)], e0


def _pow2(e):
    return Fraction(2) ** e


def packed(i, k):
    return i * (i + 1) // 2 + k


def exact_gram(proj, B):
    """(G, A): packed lower triangles (lists of Fraction) of sum proj B_i B_k and of sum proj |B_i| |B_k|."""
    p, ep = _scaled(proj)
    cols = [_scaled(b) for b in B]
    pc = [([a * b for a, b in zip(p, c)], [a * abs(b) for a, b in zip(p, c)]) for c, _ in cols]
    absc = [[abs(b) for b in c] for c, _ in cols]
    G, A = [], []
    for i in range(len(B)):
        for k in range(i + 1):
            sc = _pow2(ep + cols[i][1] + cols[k][1])
            G.append(sum(a * b for a, b in zip(pc[i][0], cols[k][0])) * sc)
            A.append(sum(a * b for a, b in zip(pc[i][1], absc[k])) * sc)
    return G, A


def gram_violations(gram, G, A, n):
    """[(i, k, got, wanted, |error|, bound)] of the returned packed `gram` outside gamma_{n+1} A."""
    bad, g = [], gamma(n + 1)
    J1 = int(round((math.sqrt(8 * len(G) + 1) - 1) / 2))
    for i in range(J1):
        for k in range(i + 1):
            e = packed(i, k)
            err = abs(Fraction(float(gram[e])) - G[e])
            if err > g * A[e]:
                bad.append((i, k, float(gram[e]), float(G[e]), float(err), float(g * A[e])))
    return bad


# ------------------------------------------------------------------------------------------------ the solve
def cholesky_solve(gram, J):
    """The loops of include/bmo.h in Python floats on the packed `gram`: (coef [J], status 0 / 2, L as a list of rows)."""
    g = [float(v) for v in gram]
    L = [[0.0] * J for _ in range(J)]
    for j in range(J):
        d = g[packed(j, j)]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not d > 0.0:
            return [math.nan] * J, 2, L
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, J):
            s = g[packed(i, j)]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = s / L[j][j]
    yv = [0.0] * J
    for i in range(J):
        s = g[packed(J, i)]
        for k in range(i):
            s = s - L[i][k] * yv[k]
        yv[i] = s / L[i][i]
    c = [0.0] * J
    for i in range(J - 1, -1, -1):
        s = yv[i]
        for k in range(i + 1, J):
            s = s - L[k][i] * c[k]
        c[i] = s / L[i][i]
    return c, 0, L


def exact_inverse(G, J):
    """The inverse of the J x J block of the packed exact G, as rows of Fractions.  The entries are dyadic: scaled by their largest
    denominator D they are integers M = D G, inverted by the fraction-free Gauss-Jordan elimination of Bareiss (every division is exact, the
    diagonal ends as det M; G is positive definite, so no pivot is zero): G^-1 = D adj(M) / det M.  The product M adj(M) = det M I is checked."""
    D = max(G[packed(i, k)].denominator for i in range(J) for k in range(i + 1))
    M = [[int(G[packed(max(i, k), min(i, k))] * D) for k in range(J)] for i in range(J)]
    A = [row[:] + [int(i == k) for k in range(J)] for i, row in enumerate(M)]
    prev = 1
    for k in range(J):
        piv = A[k][k]
        assert piv > 0
        rk = A[k]
        for i in range(J):
            if i != k:
                f = A[i][k]
                A[i] = [(piv * a - f * b) // prev for a, b in zip(A[i], rk)]
        prev = piv
    det = A[0][0]
    X = [row[J:] for row in A]
    for i in range(J):
        assert A[i][i] == det
        for k in range(J):
            assert sum(M[i][q] * X[q][k] for q in range(J)) == (det if i == k else 0)
    return [[Fraction(D * v, det) for v in row] for row in X]


def coef_bounds(gram, G, J, coef, L, Ginv=None):
    """(c exact [J], bound [J]) as Fractions: the a-posteriori bound of the module docstring."""
    Ginv = exact_inverse(G, J) if Ginv is None else Ginv
    b = [G[packed(J, k)] for k in range(J)]
    c = [sum(Ginv[i][k] * b[k] for k in range(J)) for i in range(J)]
    ch = [abs(Fraction(float(v))) for v in coef]
    g3 = gamma(3 * J + 1)
    Lf = [[abs(Fraction(v)) for v in row] for row in L]
    rhs = []
    for i in range(J):
        t = abs(Fraction(float(gram[packed(J, i)])) - b[i])
        for k in range(J):
            lo, hi = min(i, k), max(i, k)
            dg = abs(Fraction(float(gram[packed(hi, lo)])) - G[packed(hi, lo)]) + g3 * sum(Lf[i][q] * Lf[k][q] for q in range(lo + 1))
            t += dg * ch[k]
        rhs.append(t)
    return c, [sum(abs(Ginv[i][k]) * rhs[k] for k in range(J)) for i in range(J)], Ginv


def coef_violations(coef, c, bound):
    bad = []
    for j, (got, want, bd) in enumerate(zip(coef, c, bound)):
        err = abs(Fraction(float(got)) - want)
        if not err <= bd:
            bad.append((j, float(got), float(want), float(err), float(bd)))
    return bad


def fit_rms_exact(proj, E):
    """(rms to 60 decimals rounded down, bound) of sqrt(sum proj E^2 / S) for the doubles E_h, as Fractions."""
    w, e = pr._fr(proj), pr._fr(E)
    n = len(w)
    s = sum(w)
    v = sum(a * b * b for a, b in zip(w, e)) / s
    b_v = gamma(2 * n + 2) * v
    rms = sqrt_fraction(v)
    up = sqrt_fraction(b_v) + pr.EPS60
    root = rms + sqrt_fraction(max(Fraction(0), v - b_v))
    move = min(b_v / root, up) if root > 0 else up
    return rms, move + U * (rms + move) + pr.EPS60


def image_of_row_error(Ginv, proj, B, J):
    """[J] floats: an upper bound of sum_h proj_h |(G^-1 z_h)_j|, the factor by which a per-row error of the wavefront reaches coefficient j.
    Evaluated in float64 from the exact inverse rounded to doubles: the matrix-vector product of J terms commits at most
    gamma_{J+2} (|G^-1| |z_h|)_j including the rounding of G^-1's entries, which is added per row; the sum over the rows is then inflated
    by gamma_{n+2} for its own roundings."""
    Gi = np.array([[float(v) for v in row] for row in Ginv])
    Z = np.asarray(B[:J])
    p = np.asarray(proj)
    n = len(p)
    gJ = (J + 2) * 2.0 ** -53 / (1 - (J + 2) * 2.0 ** -53)
    img = np.abs(Gi @ Z) + gJ * (np.abs(Gi) @ np.abs(Z))
    gn = (n + 2) * 2.0 ** -53 / (1 - (n + 2) * 2.0 ** -53)
    return (img * p[None, :]).sum(axis=1) * (1 + gn)
