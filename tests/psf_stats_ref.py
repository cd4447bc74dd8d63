"""Helpers of the wavefront read-out tests (not a test file): the definitions of include/bmo.h "Wavefront read-out" in elementwise numpy
(which makes the per-row doubles x_h, z_h, W_h) and in fractions.Fraction on those doubles taken as data, and the derived error bounds.

Per row (numpy, one rounding per operation, left to right as the header writes them; numpy does not contract):
    x_h = ((hx - ox) * e1x + (hy - oy) * e1y) + (hz - oz) * e1z,  z_h likewise with e2
    p   = (origin + X_REF * e1) + Z_REF * e2                                   (X_REF, Z_REF: columns of the statistics under test)
    W_h = opl_h + (((px - hx) * dx + (py - hy) * dy) + (pz - hz) * dz)
The engine evaluates the same expressions, so it sums the same doubles; what is left to bound is the summation.

Bounds.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1; Lemma 3.3 for quotients:
(1 + theta_k) / (1 + theta_j) = 1 + theta_{k+j} for j <= k, theta_{k+2j} otherwise).  n rows, w_h = proj_h > 0, S = sum w_h.

  N, X_MIN .. Z_MAX, K_MIN, K_MAX   exact (comparisons of the same doubles).
  X_REF, Z_REF    the given point, or bit for bit CX, CZ of the same statistics.
  S       a sum of n positive terms in any order: each term passes at most n - 1 additions, S^ = sum w_h (1 + theta_{n-1}), so
          |S^ - S| <= gamma_{n-1} S, and S^ = S (1 + eta) with |eta| <= gamma_{n-1} (positive weights).
  CX      the numerator: one rounding of w_h * x_h and n - 1 additions, theta_n per term; the division one more (k = n + 1); the
          denominator j = n - 1 <= k.  CX^ = sum w_h x_h (1 + theta_{2n}) / S:   E_c = gamma_{2n} sum w_h |x_h| / S.
          CZ and W_MEAN (E_w, with |W_h|) have the same form.
  HWX     max_h |fl(x_h - CX^)| about the COMPUTED centroid: fl and abs are monotone, a maximum commits no rounding, so the engine's value
          equals the numpy expression on the statistics' own CX bit for bit.  HWZ likewise; W_LO, W_HI likewise about the computed W_MEAN.
  V       (the variance, W_RMS^2) per term d = fl(W_h - m^) (1), d * d (1 + e)^2 (1 + e') (3 so far), times w_h (4), n - 1 additions,
          the division (k = n + 4); denominator j = n - 1: theta_{2n+3}, covered by gamma_{2n+4}.  Exactly,
          sum w_h (W_h - m^)^2 / S = V + delta^2 with delta = m^ - m, because sum w_h (W_h - m) = 0: the mean's error enters only squared.
          |V^ - V| <= B_V := gamma_{2n+4} (V + E_w^2) + E_w^2.
  W_RMS   |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) with a >= max(0, b - B_V): the root moves by at most
          B_V / (sqrt(V) + sqrt(max(0, V - B_V))), never by more than sqrt(B_V); the correctly rounded sqrt adds u times its result.
  F       against readout_ref.psf_field_exact at (X_REF, Z_REF): B_F = psf_oracle_bound(rows, max_phase) + psf_engine_bound(rows) (derived in
          readout_ref.py for any order of the sum) + u |F| for the one rounding of the 40-digit sum to complex128.  Each component.
  STREHL  exact value |F|^2 / S^2.  With |F^ - F| <= sqrt(2) B_F =: b (both components), | |F^|^2 - |F|^2 | <= 2 |F| b + b^2.  The engine
          computes (re * re + im * im) / (S^ * S^): three roundings above (k = 3 with the quotient's: 4), below (1 + eta)^2 (1 + e):
          j = 2 (n - 1) + 1 = 2 n - 1; j > k for n >= 3, so theta_{k+2j} = theta_{4n+2} covers every n.
          B_ST = (2 |F| b + b^2) / S^2 + gamma_{4n+2} (|F| + b)^2 / S^2.
"""
import math
from fractions import Fraction

import numpy as np

import readout_ref as rr
from spot_ref import gamma, sqrt_fraction

U = Fraction(1, 2 ** 53)
STAT_N = 21
(N, S, CX, CZ, X_MIN, X_MAX, Z_MIN, Z_MAX, HWX, HWZ, X_REF, Z_REF, W_MEAN, W_RMS, W_LO, W_HI, F_RE, F_IM, STREHL, K_MIN, K_MAX) = range(STAT_N)
STAT_NAMES = ("N", "S", "CX", "CZ", "X_MIN", "X_MAX", "Z_MIN", "Z_MAX", "HWX", "HWZ", "X_REF", "Z_REF", "W_MEAN", "W_RMS", "W_LO", "W_HI", "F_RE",
              "F_IM", "STREHL", "K_MIN", "K_MAX")
EPS60 = Fraction(1, 10 ** 59)  # sqrt_fraction rounds down at 60 decimals


def _rows(rows):
    return np.asarray(rows, dtype=np.float64).reshape(-1, 9)


# ------------------------------------------------------------------------------------------------ the per-row doubles
def local_xz(rows, origin, e1, e2):
    """(x_h, z_h) [n] by the header's expression."""
    r = _rows(rows)
    o, a, b = (np.asarray(v, dtype=np.float64) for v in (origin, e1, e2))
    dx, dy, dz = r[:, 0] - o[0], r[:, 1] - o[1], r[:, 2] - o[2]
    return (dx * a[0] + dy * a[1]) + dz * a[2], (dx * b[0] + dy * b[1]) + dz * b[2]


def ref_point(origin, e1, e2, x_ref, z_ref):
    """p = (origin + X_REF * e1) + Z_REF * e2 per component."""
    o, a, b = (np.asarray(v, dtype=np.float64) for v in (origin, e1, e2))
    return (o + np.float64(x_ref) * a) + np.float64(z_ref) * b


def paths(rows, p):
    """W_h = opl_h + l_h [n] by the header's expression."""
    r = _rows(rows)
    l = ((p[0] - r[:, 0]) * r[:, 3] + (p[1] - r[:, 1]) * r[:, 4]) + (p[2] - r[:, 2]) * r[:, 5]
    return r[:, 6] + l


# ------------------------------------------------------------------------------------------------ exact values and bounds
def _fr(a):
    return [Fraction(float(v)) for v in a]


def exact_stats(x, z, W, proj):
    """The weighted sums of the doubles x_h, z_h, W_h, proj_h in exact arithmetic (W_RMS to 60 decimals, rounded down)."""
    x, z, W, w = _fr(x), _fr(z), _fr(W), _fr(proj)
    n = len(w)
    s = sum(w)
    cx, cz, m = sum(a * b for a, b in zip(w, x)) / s, sum(a * b for a, b in zip(w, z)) / s, sum(a * b for a, b in zip(w, W)) / s
    v = sum(a * (b - m) ** 2 for a, b in zip(w, W)) / s
    return dict(n=n, s=s, cx=cx, cz=cz, m=m, v=v, rms=sqrt_fraction(v), ax=sum(a * abs(b) for a, b in zip(w, x)) / s,
                az=sum(a * abs(b) for a, b in zip(w, z)) / s, aw=sum(a * abs(b) for a, b in zip(w, W)) / s)


def sum_bounds(ex):
    """(B_S, E_cx, E_cz, E_w, B_V, B_rms) of the module docstring, as Fractions."""
    n = ex["n"]
    g = gamma(2 * n)
    e_w = g * ex["aw"]
    b_v = gamma(2 * n + 4) * (ex["v"] + e_w * e_w) + e_w * e_w
    up = sqrt_fraction(b_v) + EPS60
    root = ex["rms"] + sqrt_fraction(max(Fraction(0), ex["v"] - b_v))
    move = min(b_v / root, up) if root > 0 else up
    return gamma(n - 1) * ex["s"], g * ex["ax"], g * ex["az"], e_w, b_v, move + U * (ex["rms"] + move) + EPS60


def field_bound(rows, origin, e1, e2, x_ref, z_ref, f_exact):
    """B_F: per component of F, against psf_field_exact."""
    r = _rows(rows)
    max_phase = rr.psf_max_phase(r, origin, e1, e2, [x_ref], [z_ref])
    return rr.psf_oracle_bound(r, max_phase) + rr.psf_engine_bound(r) + 2.0 ** -53 * abs(f_exact)


def strehl_bound(n, f_abs, b_f, s):
    """B_ST from |F| (float), B_F (float) and S (Fraction)."""
    f, b = Fraction(f_abs), Fraction(b_f) * Fraction(1414213563, 10 ** 9) + Fraction(b_f) / 10 ** 9  # sqrt(2) rounded up
    return (2 * f * b + b * b) / (s * s) + gamma(4 * n + 2) * (f + b) ** 2 / (s * s)


def stat_violations(got, rows, origin, e1, e2, ref=None):
    """[(name, got, wanted, |error|, bound), ...] of the statistics `got` [21] that miss their check on `rows` (empty: all inside).  ref: the
    reference point handed to the engine, None for the centroid.  No rows: N = 0 and NaN in the other twenty."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (STAT_N,)
    r = _rows(rows)
    n = len(r)
    if n == 0:
        ok = got[N] == 0 and np.isnan(got[1:]).all()
        return [] if ok else [("empty", got.tolist(), None, None, None)]
    bad = []
    if not np.isfinite(got).all():
        return [("finite", got.tolist(), None, None, None)]

    def same(k, want):
        if np.float64(got[k]).tobytes() != np.float64(want).tobytes():
            bad.append((STAT_NAMES[k], got[k], float(want), abs(got[k] - want), 0.0))

    def near(k, want, bound):
        err = abs(Fraction(float(got[k])) - Fraction(want))
        if err > bound:
            bad.append((STAT_NAMES[k], got[k], float(want), float(err), float(bound)))

    x, z = local_xz(r, origin, e1, e2)
    same(N, n)
    for k, v in ((X_MIN, x.min()), (X_MAX, x.max()), (Z_MIN, z.min()), (Z_MAX, z.max()), (K_MIN, r[:, 8].min()), (K_MAX, r[:, 8].max())):
        same(k, v)
    same(X_REF, got[CX] if ref is None else ref[0])
    same(Z_REF, got[CZ] if ref is None else ref[1])
    same(HWX, np.abs(x - got[CX]).max())
    same(HWZ, np.abs(z - got[CZ]).max())
    p = ref_point(origin, e1, e2, got[X_REF], got[Z_REF])
    W = paths(r, p)
    same(W_LO, (W - got[W_MEAN]).min())
    same(W_HI, (W - got[W_MEAN]).max())
    ex = exact_stats(x, z, W, r[:, 7])
    b_s, e_cx, e_cz, e_w, b_v, b_rms = sum_bounds(ex)
    near(S, ex["s"], b_s)
    near(CX, ex["cx"], e_cx)
    near(CZ, ex["cz"], e_cz)
    near(W_MEAN, ex["m"], e_w)
    near(W_RMS, ex["rms"], b_rms)
    f = complex(rr.psf_field_exact(r, origin, e1, e2, [got[X_REF]], [got[Z_REF]])[0, 0])
    b_f = field_bound(r, origin, e1, e2, got[X_REF], got[Z_REF], f)
    near(F_RE, f.real, Fraction(b_f))
    near(F_IM, f.imag, Fraction(b_f))
    near(STREHL, Fraction(f.real) ** 2 / ex["s"] ** 2 + Fraction(f.imag) ** 2 / ex["s"] ** 2, strehl_bound(n, abs(f), b_f, ex["s"]))
    return bad


# ------------------------------------------------------------------------------------------------ plain evaluations
def two_pass_sequential(rows, origin, e1, e2, ref=None):
    """The three passes in plain sequential float64 (one Python float operation per rounding, rows in order)."""
    r = _rows(rows)
    n = len(r)
    out = np.full(STAT_N, np.nan)
    out[N] = n
    if n == 0:
        return out
    x, z = local_xz(r, origin, e1, e2)
    w = r[:, 7].tolist()
    s = sx = sz = 0.0
    for a, b, c in zip(w, x.tolist(), z.tolist()):
        s += a
        sx += a * b
        sz += a * c
    cx, cz = sx / s, sz / s
    xr, zr = (cx, cz) if ref is None else (float(ref[0]), float(ref[1]))
    W = paths(r, ref_point(origin, e1, e2, xr, zr))
    sw = re = im = 0.0
    for a, b, k in zip(w, W.tolist(), r[:, 8].tolist()):
        sw += a * b
        re += a * math.cos(k * b)
        im += a * math.sin(k * b)
    m = sw / s
    var = 0.0
    for a, b in zip(w, W.tolist()):
        d = b - m
        var += a * (d * d)
    out[1:] = [s, cx, cz, x.min(), x.max(), z.min(), z.max(), np.abs(x - cx).max(), np.abs(z - cz).max(), xr, zr, m, math.sqrt(var / s), (W - m).min(),
               (W - m).max(), re, im, (re * re + im * im) / (s * s), r[:, 8].min(), r[:, 8].max()]
    return out


def one_pass_w_rms(rows, origin, e1, e2, x_ref, z_ref):
    """W_RMS by the textbook one-pass form sqrt((sum w W^2 - S m^2) / S) in sequential float64: what the engine must NOT do."""
    r = _rows(rows)
    W = paths(r, ref_point(origin, e1, e2, x_ref, z_ref)).tolist()
    s = sw = sw2 = 0.0
    for a, b in zip(r[:, 7].tolist(), W):
        s += a
        sw += a * b
        sw2 += a * (b * b)
    m = sw / s
    return math.sqrt(max(0.0, (sw2 - s * (m * m)) / s))


# ------------------------------------------------------------------------------------------------ inputs
LAM = 1e-6
F_LOCAL = (0.3e-3, -0.2e-3)


def tilted_pose():
    """(origin, e1, e2) of readout_ref.tilted_psf_case's detector: no component of e1 / e2 is zero."""
    import bmo_amd as bmo

    mm = 1e-3
    psfd = bmo.PSFDetector(10 * mm)
    bmo.zrotate3d(psfd, math.radians(5))
    bmo.xrotate3d(psfd, math.radians(8))
    bmo.zrotate3d(psfd, math.radians(-3))
    bmo.translate3d(psfd, [0.4 * mm, 200.13 * mm, -0.3 * mm])
    o = np.asarray(psfd.orientation(), dtype=np.float64)
    return np.asarray(psfd.position(), dtype=np.float64), o[:, 0].copy(), o[:, 2].copy()


def _cone_dirs(n, rng, e1, e2, half_angle=0.0375):
    """n unit vectors within `half_angle` of the detector's normal e1 x e2 (normalised in numpy: |d|^2 = 1 within a few u)."""
    nrm = np.cross(e1, e2)
    a, b = half_angle * rng.uniform(-1, 1, n), half_angle * rng.uniform(-1, 1, n)
    d = nrm[None, :] + a[:, None] * e1[None, :] + b[:, None] * e2[None, :]
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def synthetic_rows(n, seed, pose, two_wavelengths=False):
    """n PSF rows at the project's scales: hits within 1 um of the local point F_LOCAL, directions in an f/13 cone, opl = 0.2 m + N(0, 30 nm)
    (phases of 1.3e6 rad; with the 1 um of hit spread, 10 - 100 nm of wavefront spread), proj in (0.5, 1], k = 2 pi / 1 um (half of the rows
    2 pi / 0.8 um with two_wavelengths)."""
    origin, e1, e2 = pose
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 9))
    ab = 1e-6 * rng.uniform(-1, 1, (n, 2))
    rows[:, 0:3] = origin[None, :] + (F_LOCAL[0] + ab[:, 0])[:, None] * e1[None, :] + (F_LOCAL[1] + ab[:, 1])[:, None] * e2[None, :]
    rows[:, 3:6] = _cone_dirs(n, rng, e1, e2)
    rows[:, 6] = 0.2 + 30e-9 * rng.standard_normal(n)
    rows[:, 7] = 1.0 - 0.5 * rng.uniform(0, 1, n)
    rows[:, 8] = 2 * math.pi / LAM
    if two_wavelengths:
        rows[1::2, 8] = 2 * math.pi / 0.8e-6
    return rows


FOCUS_R, FOCUS_S_MAX = 0.2, 1e-4


def focus_rows(n, seed, pose):
    """Rows of a perfect focus: rays from a sphere of radius R about f = ref_point(F_LOCAL), aimed at f, recorded s before it:
    opl = R - s, hit = f - s * dir.  Returns (rows, f)."""
    origin, e1, e2 = pose
    rng = np.random.default_rng(seed)
    f = ref_point(origin, e1, e2, *F_LOCAL)
    rows = np.zeros((n, 9))
    d = _cone_dirs(n, rng, e1, e2)
    s = FOCUS_S_MAX * rng.uniform(0, 1, n)
    rows[:, 0:3] = f[None, :] - s[:, None] * d
    rows[:, 3:6] = d
    rows[:, 6] = FOCUS_R - s
    rows[:, 7] = 1.0 - 0.5 * rng.uniform(0, 1, n)
    rows[:, 8] = 2 * math.pi / LAM
    return rows, f


def focus_row_error(f):
    """E_row: a bound of |W_h - R| for focus_rows read at its f (p = f bit for bit: ref_point is the engine's expression).
    hit_i = fl(f_i - fl(s d_i)) is off s d_i's exact complement by u (s + |hit_i|) <= u (2 s + |f_i|); fl(p_i - hit_i) adds u s: so
    (p - hit)_i = s d_i + delta_i with |delta_i| <= u (3 s + |f_i|).  The exact dot product is s |d|^2 + sum delta_i d_i, where
    | |d|^2 - 1 | <= 4 u (two roundings of the squared norm's sum beyond the products', sqrt, divide: below 8 u s after the factor s is taken
    generously) and |sum delta_i d_i| <= u (9 s + |f|_1); the computed one adds gamma_3 s (1 + 4 u).  opl = fl(R - s) and W = fl(opl + l) add
    u R each, and R - s + s = R exactly.  Sum: u (2 R + |f|_1 + 21 s), stated as 2 u (R + |f|_1 + 11 s)."""
    return 2 * float(U) * (FOCUS_R + float(np.abs(f).sum()) + 11 * FOCUS_S_MAX)


def offset_wavefront(n=4000, seed=11, pose=None):
    """W = 0.2 m + N(0, 10 nm): the one-pass variance loses every digit here."""
    pose = tilted_pose() if pose is None else pose
    rows, f = focus_rows(n, seed, pose)
    rows[:, 6] += 10e-9 * np.random.default_rng(seed + 1).standard_normal(n)
    return rows, pose
