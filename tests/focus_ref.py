"""Helpers of the through-focus read-out tests (not a test file): 40-digit evaluations written from the formulas of include/bmo.h
"Through-focus read-out" alone, and the error bounds of the engine's arithmetic, derived here and not fitted.

1. through_focus_exact: plane m of the stack,

       F_m(x, z) = sum_h proj_h cis(k_h (opl_h + dot(origin + x e1 + z e2 + d_m - pos_h, dir_h))),

   every input the exact value of its double; d_m is added exactly, NOT folded into a rounded origin.  No factorisation into two cis: it is
   the field of readout_ref.psf_field_exact at the exact point p + d_m.

2. focus_stats_exact: every row propagated along its direction to the plane through o_m = origin + offsets[m] axis (exact) with normal
   e1 x e2 (exact), its local coordinates there, and the weighted statistics of them, all at 40 digits.

3. The bounds.  u = 2^-53, gamma_k = k u / (1 - k u); S = sum proj.

   The stack against (1), each component of the field (stack_bound).  Per row, in units of proj_h, to first order in u; the second-order
   terms are below 1e-12 of the first-order ones and the constants below are rounded up by far more than that.
     a. the argument of the point factor, phase = fl(k * fl(opl + l)) with l from the rounded point:
          p_c = fl(fl(o_c + fl(x e1_c)) + fl(z e2_c)) is off by at most u (|x e1_c| + |z e2_c| + |o_c + x e1_c| + |p_c|) <= 2 u (|o_c| + |x| + |z|);
          a_c = fl(p_c - pos_c) adds u |a_c|; the dot product of three terms adds gamma_3 sum |a_c dir_c|.  With |dir|_2 = 1 (1 + few u):
          |dl| <= 2 u (|o|_2 + 2 (|x| + |z|)) + 4 u |a|_1.   The sum opl + l and the product with k add u |phase| each:
          |dphase| <= 2 u |phase| + k (2 u |o|_2 + 4 u (|x| + |z|) + 4 u |a|_1)                                         (arg_point)
     b. the argument of the plane factor, fl(k * g), g = fl(fl(d_x dir_x + d_y dir_y) + d_z dir_z): gamma_3 sum |d_c dir_c| <= 3 u |d|_1, the
        product with k adds u k |g| <= u k |d|_1:   |darg| <= 4 u k |d|_1                                                (arg_plane)
        A radian of argument moves cis by at most one unit, in modulus and so in each component.
     c. the two device sincos: 4 ulp per component (the OpenCL FP64 bound the existing read-out bounds use), an ulp of a value in
        [-1, 1] is at most 2 u: each component within 8 u, the complex value within 8 sqrt(2) u = 11.32 u; the other factor has modulus 1,
        so the term moves by 11.32 u for each of the two: 22.63 u.
     d. t_re = fl(proj c), t_im = fl(proj s): each within u of its value: the complex t within u |t|: 1 u.
     e. the complex multiply-add, re = fl(fl(t_re u_re) - fl(t_im u_im)): gamma_2 (|t_re u_re| + |t_im u_im|) <= 2 u |t| |u|: 2 u.
     c + d + e = 25.63 u, stated as C_TERM = 27 u.
     f. the sum over H rows, in any order: each term passes at most H - 1 additions: gamma_{H-1} sum |term| <= (H + 1) u S.
     g. the 40-digit value rounded to complex128: u |F|.
   B = (arg_point + arg_plane + 27 u + (H + 1) u) S + u |F|.

   bmo_psf_intensity against the exact field at its own (double) origin (intensity_bound): the same without b and with one sincos
   (11.32 u), d, and one addition per component in place of e (absorbed in f): 12.32 u, stated as 14 u.

   The statistics against (2) (stat_bounds).  L: the largest |coordinate| of a hit, a plane origin or a propagated point; R: the largest of
   |o_m - pos|_2, |s| and |q - o_m|_1 (the millimetre scale of the problem); kappa = 1 / min |den| >= 1.
     o_m:  fl(o_c + fl(off a_c)) is off by at most u (|off a_c| + |o_mc|) <= 2 u L per component.
     b_c = fl(o_mc - pos_c): 2 u L + u |b_c|.    nrm = e1 x e2 in doubles: each component within gamma_2 (|e1 e2| + |e1 e2|) <= 2 u,
     |dnrm|_2 <= 3.5 u.
     num = fl(dot(b, nrm)): sqrt(3) (2 u L + u R) + 3.5 u R + gamma_3 R <= 3.5 u L + 8.3 u R;   den = fl(dot(dir, nrm)): 3.5 u + 3 u = 6.5 u
     s = fl(num / den): kappa (3.5 u L + 8.3 u R) + 6.5 u kappa |s| + u |s| <= kappa^2 (3.5 u L + 16 u R)
     q_c = fl(pos_c + fl(s dir_c)): |ds| + u R + u L;   fl(q_c - o_mc): adds 2 u L + u R
     x = fl(dot(q - o_m, e1)): sqrt(3) (|ds| + 3 u L + 2 u R) + gamma_3 R <= kappa^2 (11.3 u L + 35 u R), stated as
     E_row = u kappa^2 (12 L + 36 R): the engine's x and z of every row and plane are within E_row of the exact ones.
     S          gamma_{n-1} S (positive terms, any order).
     X_MIN ..   E_row (an extremum of values that each moved by at most E_row moves by at most E_row).
     CX, CZ     E_c = E_row + gamma_{2n} (sum proj (|x| + E_row)) / S: the weighted mean of moved values moves by at most E_row; the sum of
                products and the quotient as in psf_stats_ref (theta_{2n}).
     HWX, HWZ   e = E_row + E_c, and the subtraction's rounding: e + u (HW + e).
     RMS_R      the engine's (ax, az) of a row is within (e_x, e_z) of the exact (x - CX, z - CZ), plus u of itself: the radius vector moves by
                at most e_r = sqrt(e_x^2 + e_z^2) (1 + u) + 2 u MAX_R; the weighted root mean square is a norm: it moves by at most e_r.  The
                floating evaluation of sqrt(sum proj r2 / S): r2 theta_3, the product theta_1, n - 1 additions, the quotient with S^
                (theta_{n-1}), the root: inside gamma_{2n+5} relative.   B = e_r + gamma_{2n+5} (RMS_R + e_r).
     MAX_R      e_r + 3 u (MAX_R + e_r)   (r2 theta_3, halved by the root, the root's own u).
"""
import math

import numpy as np

import readout_ref as rr

U = 2.0 ** -53
C_TERM = 27.0
C_TERM_DIRECT = 14.0
STAT_N = 12
(N, S, CX, CZ, X_MIN, X_MAX, Z_MIN, Z_MAX, HWX, HWZ, RMS_R, MAX_R) = range(STAT_N)
STAT_NAMES = ("N", "S", "CX", "CZ", "X_MIN", "X_MAX", "Z_MIN", "Z_MAX", "HWX", "HWZ", "RMS_R", "MAX_R")


def gamma(k):
    return k * U / (1 - k * U)


def _rows(rows):
    return np.asarray(rows, dtype=np.float64).reshape(-1, 9)


def _ex(mp, a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]  # a double is a dyadic rational: mpf(float) is exact


# ------------------------------------------------------------------------------------------------ the stack
def through_focus_exact(hits, origin, e1, e2, displacements, xs, zs):
    """F[m, i, j] at (xs[i], zs[j]) of plane m as complex128 (the 40-digit sum rounded once at the end)."""
    import mpmath as mp

    d = np.asarray(displacements, dtype=np.float64).reshape(-1, 3)
    with mp.workdps(40):
        o, a1, a2 = _ex(mp, origin), _ex(mp, e1), _ex(mp, e2)
        rows = [_ex(mp, r) for r in _rows(hits)]
        out = np.zeros((len(d), len(xs), len(zs)), dtype=np.complex128)
        for m, dm in enumerate(d):
            dm = _ex(mp, dm)
            for i, x in enumerate(_ex(mp, xs)):
                for j, z in enumerate(_ex(mp, zs)):
                    p = [o[k] + x * a1[k] + z * a2[k] + dm[k] for k in range(3)]
                    acc = mp.mpc(0)
                    for r in rows:
                        l = mp.fsum((p[k] - r[k]) * r[3 + k] for k in range(3))
                        acc += r[7] * mp.expjpi(r[8] * (r[6] + l) / mp.pi)
                    out[m, i, j] = complex(acc)
    return out


def propagate_exact(hits, origin, e1, e2, shift):
    """Rows recorded on the detector plane (origin, e1, e2) propagated exactly to the plane through origin + shift with the same normal:
    hit' = hit + s dir, opl' = opl + s.  `hits`: doubles [H, 9], or a list of mpf rows (directions normalised at 40 digits, say).  Returns mpf
    rows [[9 mpf], ...], not rounded; call it inside mp.workdps(40)."""
    import mpmath as mp

    o, a1, a2, sh = _ex(mp, origin), _ex(mp, e1), _ex(mp, e2), _ex(mp, shift)
    nrm = [a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]]
    out = []
    for r in (hits if isinstance(hits, list) else [_ex(mp, r) for r in _rows(hits)]):
        s = mp.fsum((o[k] + sh[k] - r[k]) * nrm[k] for k in range(3)) / mp.fsum(r[3 + k] * nrm[k] for k in range(3))
        out.append([r[0] + s * r[3], r[1] + s * r[4], r[2] + s * r[5], r[3], r[4], r[5], r[6] + s, r[7], r[8]])
    return out


def field_exact_mp(rows_mp, p_mp):
    """sum_h proj cis(k (opl + dot(p - pos, dir))) of mpf rows at the mpf point p, as an mpc (not rounded)."""
    import mpmath as mp

    acc = mp.mpc(0)
    for r in rows_mp:
        l = mp.fsum((p_mp[k] - r[k]) * r[3 + k] for k in range(3))
        acc += r[7] * mp.expjpi(r[8] * (r[6] + l) / mp.pi)
    return acc


def _geometry(hits, origin, e1, e2, xs, zs):
    """(max |phase|, max (|x| + |z|), max |p - pos|_1) over the grid and the rows, in plain doubles (they only scale a bound)."""
    h = _rows(hits)
    o, a1, a2 = (np.asarray(v, dtype=np.float64) for v in (origin, e1, e2))
    p = o[None, None, :] + np.asarray(xs)[:, None, None] * a1[None, None, :] + np.asarray(zs)[None, :, None] * a2[None, None, :]
    a1n = np.abs(p[:, :, None, :] - h[None, None, :, 0:3]).sum(axis=3).max()
    return rr.psf_max_phase(h, origin, e1, e2, xs, zs), float(np.abs(xs).max() + np.abs(zs).max()), float(a1n)


def arg_point(hits, origin, e1, e2, xs, zs):
    """a. of the module docstring: the largest error of the argument of the point factor, in radians."""
    h = _rows(hits)
    phase, xz, a1n = _geometry(h, origin, e1, e2, xs, zs)
    return 2 * U * phase + float(h[:, 8].max()) * U * (2 * float(np.linalg.norm(origin)) + 4 * xz + 4 * a1n)


def stack_bound(hits, origin, e1, e2, d, xs, zs, f_abs=0.0):
    """B of the module docstring for the plane displaced by d (its largest |F| over the checked points as f_abs): each component."""
    h = _rows(hits)
    if len(h) == 0:
        return 0.0
    k_max, s = float(h[:, 8].max()), float(h[:, 7].sum())
    arg_plane = 4 * U * k_max * float(np.abs(d).sum())
    return (arg_point(h, origin, e1, e2, xs, zs) + arg_plane + C_TERM * U + (len(h) + 1) * U) * s * (1 + 1e-9) + U * f_abs


def intensity_bound(hits, origin, e1, e2, xs, zs, f_abs=0.0):
    """bmo_psf_intensity at the double origin `origin` against the exact field there: each component."""
    h = _rows(hits)
    if len(h) == 0:
        return 0.0
    return (arg_point(h, origin, e1, e2, xs, zs) + C_TERM_DIRECT * U + (len(h) + 1) * U) * float(h[:, 7].sum()) * (1 + 1e-9) + U * f_abs


def origin_offset(origin, d, moved):
    """|moved - (origin + d)|_1 with the three doubles taken exactly: how far the double `moved` is from the exact displaced origin."""
    import mpmath as mp

    with mp.workdps(40):
        o, dd, mv = _ex(mp, origin), _ex(mp, d), _ex(mp, moved)
        return float(mp.fsum(abs(mv[k] - (o[k] + dd[k])) for k in range(3))) * (1 + 1e-9)


def origin_shift_term(hits, origin, d, moved):
    """k_max S |moved - (origin + d)|_1: what reading at the double `moved` instead of the exact origin + d changes, at most."""
    h = _rows(hits)
    return float(h[:, 8].max()) * float(h[:, 7].sum()) * origin_offset(origin, d, moved)


# ------------------------------------------------------------------------------------------------ the statistics
def focus_stats_exact(hits, origin, e1, e2, axis, offsets):
    """One dict per plane: the exact statistics (floats of 40-digit values) and the scales the bounds need."""
    import mpmath as mp

    h = _rows(hits)
    out = []
    with mp.workdps(40):
        o, a1, a2, ax = _ex(mp, origin), _ex(mp, e1), _ex(mp, e2), _ex(mp, axis)
        nrm = [a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]]
        rows = [_ex(mp, r) for r in h]
        dens = [mp.fsum(r[3 + k] * nrm[k] for k in range(3)) for r in rows]
        for off in _ex(mp, offsets):
            om = [o[k] + off * ax[k] for k in range(3)]
            xs, zs, big_l, big_r, s_max = [], [], max(abs(v) for v in om), mp.mpf(0), mp.mpf(0)
            for r, den in zip(rows, dens):
                b = [om[k] - r[k] for k in range(3)]
                s = mp.fsum(b[k] * nrm[k] for k in range(3)) / den
                q = [r[k] + s * r[3 + k] for k in range(3)]
                xs.append(mp.fsum((q[k] - om[k]) * a1[k] for k in range(3)))
                zs.append(mp.fsum((q[k] - om[k]) * a2[k] for k in range(3)))
                big_l = max(big_l, max(abs(v) for v in q), max(abs(r[k]) for k in range(3)))
                s_max = max(s_max, abs(s))
                big_r = max(big_r, mp.sqrt(mp.fsum(v * v for v in b)), abs(s), mp.fsum(abs(q[k] - om[k]) for k in range(3)))
            w = [r[7] for r in rows]
            s_sum = mp.fsum(w)
            cx, cz = mp.fsum(a * b for a, b in zip(w, xs)) / s_sum, mp.fsum(a * b for a, b in zip(w, zs)) / s_sum
            r2 = [(x - cx) ** 2 + (z - cz) ** 2 for x, z in zip(xs, zs)]
            out.append(dict(n=len(rows), s=float(s_sum), cx=float(cx), cz=float(cz), x_min=float(min(xs)), x_max=float(max(xs)), z_min=float(min(zs)),
                            z_max=float(max(zs)), hwx=float(max(abs(x - cx) for x in xs)), hwz=float(max(abs(z - cz) for z in zs)),
                            rms_r=float(mp.sqrt(mp.fsum(a * b for a, b in zip(w, r2)) / s_sum)), max_r=float(mp.sqrt(max(r2))),
                            ax=float(mp.fsum(a * abs(b) for a, b in zip(w, xs)) / s_sum), az=float(mp.fsum(a * abs(b) for a, b in zip(w, zs)) / s_sum),
                            L=float(big_l), R=float(big_r), s_max=float(s_max), kappa=float(1 / min(abs(v) for v in dens))))
    return out


def stat_bounds(ex):
    """{column: bound} of the module docstring for one plane's exact statistics `ex`."""
    n = ex["n"]
    e_row = U * ex["kappa"] ** 2 * (12 * ex["L"] + 36 * ex["R"])
    e_cx, e_cz = e_row + gamma(2 * n) * (ex["ax"] + e_row), e_row + gamma(2 * n) * (ex["az"] + e_row)
    ex_, ez_ = e_row + e_cx, e_row + e_cz
    e_r = math.hypot(ex_, ez_) * (1 + U) + 2 * U * ex["max_r"]
    return {N: 0.0, S: gamma(n - 1) * ex["s"], CX: e_cx, CZ: e_cz, X_MIN: e_row, X_MAX: e_row, Z_MIN: e_row, Z_MAX: e_row,
            HWX: ex_ + U * (ex["hwx"] + ex_), HWZ: ez_ + U * (ex["hwz"] + ez_), RMS_R: e_r + gamma(2 * n + 5) * (ex["rms_r"] + e_r),
            MAX_R: e_r + 3 * U * (ex["max_r"] + e_r)}


def stat_violations(got, ex):
    """[(name, got, wanted, |error|, bound), ...] of the statistics `got` [12] of one plane that miss their bound against `ex`."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (STAT_N,)
    if not np.isfinite(got).all():
        return [("finite", got.tolist(), None, None, None)]
    want = {N: ex["n"], S: ex["s"], CX: ex["cx"], CZ: ex["cz"], X_MIN: ex["x_min"], X_MAX: ex["x_max"], Z_MIN: ex["z_min"], Z_MAX: ex["z_max"],
            HWX: ex["hwx"], HWZ: ex["hwz"], RMS_R: ex["rms_r"], MAX_R: ex["max_r"]}
    bounds = stat_bounds(ex)
    # the exact value itself is given as its nearest double: half an ulp of it on top
    return [(STAT_NAMES[k], got[k], want[k], abs(got[k] - want[k]), bounds[k]) for k in range(STAT_N) if abs(got[k] - want[k]) > bounds[k] + U * abs(want[k])]


# ------------------------------------------------------------------------------------------------ restatements of the engine's constants
def _source_int(pattern, what):
    import re

    m = re.search(pattern, open(rr.READOUT_SOURCE).read())
    assert m, what + " not found in " + rr.READOUT_SOURCE
    return int(m.group(1))


def source_focus_mp():
    """PSF_FOCUS_MP, the planes per chunk of the stack, as the engine's source states it."""
    return _source_int(r"#define\s+BMO_PSF_FOCUS_MP\s+(\d+)", "BMO_PSF_FOCUS_MP")


def source_focus_stat_mp():
    return _source_int(r"constexpr\s+int\s+FOCUS_STAT_MP\s*=\s*(\d+)\s*;", "FOCUS_STAT_MP")


# ------------------------------------------------------------------------------------------------ the rows of two solves compared
def row_discrepancy(rows_a, rows_b, origin, e1, e2, shift):
    """(path, position): how far the recorded rows_b (a second solve with the detector moved by `shift`) are from rows_a propagated exactly to that plane, as
    a path length in metres: the largest, over the rows, of
        |opl_b - opl'| + |dot(pos_b - pos', dir_a)| + reach |dir_b - dir_a|_2 + |s| |1 - |dir_a|^2|
    with (pos', opl') = (pos + s dir, opl + s) the exact propagation of row a.  The first two terms are the path mismatch and the lateral
    mismatch projected on the direction; the third covers a direction that differs, reach = 1e-2 m bounding |p - pos| for every sample point
    of the 10 mm detector (its half-diagonal is 7.1 mm); the fourth is what the identity of the header loses where a recorded direction is a
    unit vector only to rounding: opl' + dot(p - pos', dir) = opl + dot(p - pos, dir) + s (1 - |dir|^2).  `position` is the largest
    |pos_b - pos'|_2, what the spot statistics of the two differ by at most."""
    import mpmath as mp

    a, b = _rows(rows_a), _rows(rows_b)
    assert a.shape == b.shape
    worst, worst_pos = 0.0, 0.0
    with mp.workdps(40):
        moved = propagate_exact(a, origin, e1, e2, shift)
        for r0, ra, rb in zip(a, moved, b):
            rb = _ex(mp, rb)
            dp = [rb[k] - ra[k] for k in range(3)]
            ddir = mp.sqrt(mp.fsum((rb[3 + k] - ra[3 + k]) ** 2 for k in range(3)))
            unit = abs(ra[6] - mp.mpf(float(r0[6]))) * abs(1 - mp.fsum(ra[3 + k] ** 2 for k in range(3)))
            worst = max(worst, float(abs(rb[6] - ra[6]) + abs(mp.fsum(dp[k] * ra[3 + k] for k in range(3))) + mp.mpf("1e-2") * ddir + unit))
            worst_pos = max(worst_pos, float(mp.sqrt(mp.fsum(v * v for v in dp))))
    return worst * (1 + 1e-9), worst_pos * (1 + 1e-9)
