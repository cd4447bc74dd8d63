"""Helpers of the OPD map tests (not a test file): include/bmo.h "OPD map read-out" restated in elementwise numpy, the exact per-bin mean
of the same per-row doubles, and the derived bound between the two.

The restatement takes the per-row doubles of zernike_ref (proj_h, x_h, y_h, D_h at the X_REF .. W_MEAN the call returned) and the residual
E_h = D_h - F_h of zernike_ref.residual, then evaluates the header's bin rule, shifts, q_h, p_h, the integer sums (np.add.at on int64) and the
finish expressions.  The engine evaluates the same FP64 expressions and integer sums have no order: every output of the map equals the
restatement exactly, bin-edge decisions included (no margin is needed: both sides compare the same doubles).

The bound.  u = 2^-53.  Take a bin with the rows h of `count`, A = sum proj_h E_h and B = sum proj_h exactly (of the doubles), m = A / B.
  q_h = rint(fl(proj_h E_h) 2^sh_q): the scaling by a power of two is exact, rint moves by at most 1/2, the product carries u |proj_h E_h|:
      |Q 2^-sh_q - A| <= count (2^-sh_q / 2 + u MQ)          =: d_A       (MQ = max |proj E| over all rows)
  p_h = rint(proj_h 2^sh_p), no product:   |P 2^-sh_p - B| <= count 2^-sh_p / 2      =: d_B
  (double)Q and (double)P round once each, the scalings are exact:  A^ = fl(Q) 2^-sh_q, w^ = fl(P) 2^-sh_p with
      |A^ - A| <= e_A = d_A + u |Q| 2^-sh_q,      |w^ - B| <= e_B = d_B + u |P| 2^-sh_p.
  A^ / w^ - A / B = ((A^ - A) B - A (w^ - B)) / (w^ B):     |A^ / w^ - m| <= r = (e_A + |m| e_B) / |w^|,
  and the division rounds once:  |opd - m| <= r + u (|m| + r).
"""
import math
from fractions import Fraction

import numpy as np

import psf_stats_ref as pr
import zernike_ref as zr

U = Fraction(1, 2 ** 53)
INFO_N = 20
(N, STATUS, S, X_REF, Z_REF, U0, V0, RHO, W_MEAN, E_RMS, E_LO, E_HI, N_OUT, N_OUTSIDE, N_BAD, N_FILLED, SH_Q, SH_P, MAP_LO, MAP_HI) = range(INFO_N)
INT_COLUMNS = (N, STATUS, N_OUT, N_OUTSIDE, N_BAD, N_FILLED, SH_Q, SH_P)
MAX_N = 4096
LDS_BINS = 4096  # OPD_LDS_BINS of csrc/bmo_readout.inc.hpp (test_opd_ref.py reads it from the source)


def bins(x, y, n):
    """(inside [rows] bool, key [rows] int64 = i + n j; -1 outside): the rule of bmo_spot_image on (-1, 1, -1, 1) with sx = n / 2.0"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (x >= -1.0) & (x <= 1.0) & (y >= -1.0) & (y <= 1.0)
    sx = n / 2.0
    xi, yi = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    i = np.minimum(np.floor((xi + 1.0) * sx).astype(np.int64), n - 1)
    j = np.minimum(np.floor((yi + 1.0) * sx).astype(np.int64), n - 1)
    return inside, np.where(inside, i + n * j, -1)


def shift(m, b):
    """sh(M) for N <= 2^b rows"""
    if m == 0.0:
        return 0
    return int(min(max(60 - b - (math.frexp(m)[1] - 1), -1000), 1000))


def rows_of(rows, pose, info, order, coef):
    """(proj, E, x, y) of the rows at the doubles `info` returned; coef None: nothing removed (order 0, c_0 = 0)"""
    c = np.zeros(zr.n_terms(order)) if coef is None else np.asarray(coef, dtype=np.float64)
    with np.errstate(all="ignore"):
        proj, B, x, y = zr.columns(rows, pose, info, order)
        return proj, zr.residual(B, c), x, y


def restate(proj, E, x, y, n):
    """The map of rows with a usable RHO, from the per-row doubles: dict of opd, weight, count, raw (flat, bin i + n j) and the info columns
    the map adds (N_OUT .. MAP_HI) by index."""
    rows = len(proj)
    inside, key = bins(x, y, n)
    with np.errstate(all="ignore"):
        pe = proj * E
        bad = ~(np.isfinite(proj) & np.isfinite(pe))
        t = x * x + y * y
        n_out = int((t > 1.0).sum())
    count = np.zeros(n * n, dtype=np.int64)
    np.add.at(count, key[inside], 1)
    out = {N_OUT: n_out, N_OUTSIDE: rows - int(inside.sum()), N_BAD: int(bad.sum()), N_FILLED: int((count > 0).sum()), "count": count, "key": key}
    Q, P = np.zeros(n * n, dtype=np.int64), np.zeros(n * n, dtype=np.int64)
    if bad.any():
        out.update({STATUS: 2, SH_Q: math.nan, SH_P: math.nan, MAP_LO: math.nan, MAP_HI: math.nan, "opd": np.full(n * n, np.nan), "weight": np.full(n * n, np.nan),
                    "raw": np.stack([Q, P], axis=1)})
        return out
    b = (rows - 1).bit_length()
    mq, mp = float(np.abs(pe).max()), float(np.abs(proj).max())
    sh_q, sh_p = shift(mq, b), shift(mp, b)
    q = np.rint(pe * math.ldexp(1.0, sh_q)).astype(np.int64)
    p = np.rint(proj * math.ldexp(1.0, sh_p)).astype(np.int64)
    np.add.at(Q, key[inside], q[inside])
    np.add.at(P, key[inside], p[inside])
    weight = P.astype(np.float64) * math.ldexp(1.0, -sh_p)
    with np.errstate(all="ignore"):
        opd = np.where((count > 0) & (P != 0), (Q.astype(np.float64) * math.ldexp(1.0, -sh_q)) / weight, np.nan)
    seen = opd[~np.isnan(opd)]
    out.update({STATUS: 0, SH_Q: sh_q, SH_P: sh_p, MAP_LO: seen.min() + 0.0 if len(seen) else math.nan, MAP_HI: seen.max() + 0.0 if len(seen) else math.nan,
                "opd": opd, "weight": weight, "raw": np.stack([Q, P], axis=1), "q": q, "p": p, "mq": mq, "mp": mp})
    return out


def exact_means(proj, E, key, n):
    """{bin: (m, A, B)}: the exact mean sum proj E / sum proj of the rows the restatement put there, as Fractions"""
    w, e = pr._fr(proj), pr._fr(E)
    acc = {}
    for h, k in enumerate(key.tolist()):
        if k >= 0:
            a, b = acc.get(k, (Fraction(0), Fraction(0)))
            acc[k] = (a + w[h] * e[h], b + w[h])
    return {k: (a / b, a, b) for k, (a, b) in acc.items() if b != 0}


def bin_bound(m, cnt, Q, P, sh_q, sh_p, mq):
    """the bound of |opd_b - m| of the module docstring, a Fraction"""
    iq, ip = Fraction(2) ** -sh_q, Fraction(2) ** -sh_p
    e_a = cnt * (iq / 2 + U * Fraction(mq)) + U * abs(Q) * iq
    e_b = cnt * ip / 2 + U * abs(P) * ip
    w = Fraction(float(np.float64(P))) * ip
    r = (e_a + abs(m) * e_b) / abs(w)
    return r + U * (abs(m) + r)


def map_violations(opd, R, proj, E, n):
    """([(bin, got, wanted, |error|, bound)] of the flat map `opd` outside the bound about the exact means, the largest bound) for the
    restatement R of the same rows"""
    bad, worst = [], Fraction(0)
    ex = exact_means(proj, E, R["key"], n)
    for k, (m, a, b) in ex.items():
        if R["raw"][k, 1] == 0:
            continue
        bd = bin_bound(m, int(R["count"][k]), int(R["raw"][k, 0]), int(R["raw"][k, 1]), R[SH_Q], R[SH_P], R["mq"])
        worst = max(worst, bd)
        err = abs(Fraction(float(opd[k])) - m) if np.isfinite(opd[k]) else None
        if err is None or err > bd:
            bad.append((k, float(opd[k]), float(m), None if err is None else float(err), float(bd)))
    return bad, worst, ex
