"""Helpers of the Spotdetector read-out tests (not a test file): the binning rule in numpy, exact statistics in fractions.Fraction, a
restatement of the engine's spot_splits, and the derived error bounds of the statistics.

Binning rule (include/bmo.h "Spot read-out"), window (x0, x1, z0, z1), sx = nx / (x1 - x0), sz = nz / (z1 - z0) in FP64:
    inside  iff  x >= x0 and x <= x1 and z >= z0 and z <= z1      (plain compares: a NaN is outside, the upper edge is closed)
    i = min(int64(floor((x - x0) * sx)), nx - 1),   j likewise,   bin = i + nx * j
Counts are integers: the image does not depend on the order of the rows, so the engine is held to exact equality with `bin_rule`.

Statistics (BMO_SPOT_STAT_*): two passes, centroid first, then central moments about the COMPUTED centroid.  With u = 2^-53,
gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 3.1: a product of k factors (1 + e_i), |e_i| <= u,
is 1 + theta with |theta| <= gamma_k), n rows, A_x = sum |x_i|, exact centroid c, computed centroid c^ = c + delta:

  CX     a sum of n terms in ANY order commits n - 1 roundings per term at most, the division one more: c^ = sum x_i (1 + theta_i) / n with
         |theta_i| <= gamma_n, so |delta_x| <= gamma_n A_x / n <= E_cx := gamma_{n+1} A_x / n.   (Lanes without rows add +0: exact.)
  MXX    the engine forms d_i = fl(x_i - c^), fl(d_i * d_i) (factors (1+e)^2 (1+e'): three roundings), sums the n non-negative terms in some
         order (n - 1) and divides (1): M^ = (1/n) sum (x_i - c^)^2 (1 + theta_i), |theta_i| <= gamma_{n+3}.  Exactly,
         (1/n) sum (x_i - c^)^2 = m + delta^2 because sum (x_i - c) = 0: the centroid error enters only as delta^2.  Hence
         |M^ - m| <= gamma_{n+3} (m + E_c^2) + E_c^2.
  MXZ    the same with signed terms: (1/n) sum (x_i - c^x)(z_i - c^z) = m_xz + delta_x delta_z, and
         |(x_i - c^x)(z_i - c^z)| <= (|x_i - c_x| + E_cx)(|z_i - c_z| + E_cz), so with S = (1/n) sum of that product
         |M^ - m_xz| <= gamma_{n+3} S + E_cx E_cz.
  RMS_R  s^ = fl(M^xx + M^zz) differs from s = m_xx + m_zz by at most D = (B_xx + B_zz) + u (s + B_xx + B_zz).
         |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) and a >= max(0, b - D), so the square root moves by at most
         D / (sqrt(s) + sqrt(max(0, s - D))) (for D << s: D / (2 sqrt(s)), HALF the relative bound of the sum) and never by more than sqrt(D);
         the correctly rounded sqrt adds u times its result.
  GEO_R  the distance of a point to c^ differs from its distance to c by at most |delta| <= H := hypot(E_cx, E_cz) (triangle inequality), and
         so do the maxima.  fl(fl(d_x^2) + fl(d_z^2)) carries four roundings on r^2, the square root halves them and adds one:
         |G^ - geo| <= H + gamma_4 (geo + H).
  N, X_MIN, X_MAX, Z_MIN, Z_MAX: exact.

`spot_splits` restates the function of that name in csrc/bmo_readout.inc.hpp; the tests use it ONLY to assert that a chosen row count reaches
the code path it was chosen for, never to compute an expected value.
"""
import math
import os
import re
from fractions import Fraction

import numpy as np

U = Fraction(1, 2 ** 53)
STAT_N = 12
N, CX, CZ, X_MIN, X_MAX, Z_MIN, Z_MAX, MXX, MZZ, MXZ, RMS_R, GEO_R = range(STAT_N)
STAT_NAMES = ("N", "CX", "CZ", "X_MIN", "X_MAX", "Z_MIN", "Z_MAX", "MXX", "MZZ", "MXZ", "RMS_R", "GEO_R")
LDS_BINS = 16384  # images of up to this many bins are accumulated in LDS, larger ones in global memory
READOUT_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "beamletoptics.jl_amd", "csrc", "bmo_readout.inc.hpp")


def _rows2d(rows):
    r = np.asarray(rows, dtype=np.float64)
    return r if r.ndim == 2 else r.reshape(-1, 2)


# ------------------------------------------------------------------------------------------------ the binning rule
def bin_rule(rows, window, nx, nz):
    """(image int64 [nx, nz] indexed [i, j], outside) of rows [n, >= 2] (x in column 0, z in column 1)."""
    r = _rows2d(rows)
    x, z = r[:, 0], r[:, 1]
    x0, x1, z0, z1 = (np.float64(v) for v in window)
    sx, sz = np.float64(nx) / (x1 - x0), np.float64(nz) / (z1 - z0)
    inside = (x >= x0) & (x <= x1) & (z >= z0) & (z <= z1)
    xi, zi = x[inside], z[inside]
    i = np.minimum(np.floor((xi - x0) * sx).astype(np.int64), nx - 1)
    j = np.minimum(np.floor((zi - z0) * sz).astype(np.int64), nz - 1)
    image = np.bincount(i + nx * j, minlength=nx * nz).astype(np.int64).reshape(nz, nx).T.copy()
    return image, int(len(r) - inside.sum())


def bin_exact(x, z, window, nx, nz):
    """Classification of one row in exact arithmetic: None outside, else (i, j, tx, tz) with the exact bin coordinates tx, tz (Fractions)."""
    x0, x1, z0, z1 = (Fraction(float(v)) for v in window)
    if not (math.isfinite(x) and math.isfinite(z)):
        return None
    fx, fz = Fraction(float(x)), Fraction(float(z))
    if not (x0 <= fx <= x1 and z0 <= fz <= z1):
        return None
    tx, tz = (fx - x0) * nx / (x1 - x0), (fz - z0) * nz / (z1 - z0)
    return min(math.floor(tx), nx - 1), min(math.floor(tz), nz - 1), tx, tz


# ------------------------------------------------------------------------------------------------ work splitting
def _cdiv(a, b):
    return (a + b - 1) // b


def source_spot_constants():
    """(SPOT_MIN_SPLIT, SPOT_MAX_SPLITS, SPOT_LDS_BINS) as the engine's source states them."""
    text = open(READOUT_SOURCE).read()
    out = []
    for name in ("SPOT_MIN_SPLIT", "SPOT_MAX_SPLITS", "SPOT_LDS_BINS"):
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\d+)\s*;", text)
        assert m, name + " not found in " + READOUT_SOURCE
        out.append(int(m.group(1)))
    return tuple(out)


SPOT_MIN_SPLIT, SPOT_MAX_SPLITS = 2048, 2048


def spot_splits(n_rows):
    """(n_splits, rows_per_split) of a spot read-out of n_rows rows: splits of at least SPOT_MIN_SPLIT rows, at most SPOT_MAX_SPLITS of them,
    each a multiple of 256 rows."""
    n_splits = max(1, min(_cdiv(n_rows, SPOT_MIN_SPLIT), SPOT_MAX_SPLITS))
    per = max(256, _cdiv(_cdiv(n_rows, n_splits), 256) * 256)
    return (_cdiv(n_rows, per) if n_rows > 0 else 1), per


def smallest_ragged_three_splits():
    """The smallest row count that spot_splits cuts into at least 3 splits whose last is shorter than the others."""
    n = 1
    while True:
        ns, per = spot_splits(n)
        if ns >= 3 and n % per:
            return n
        n += 1


# ------------------------------------------------------------------------------------------------ exact statistics and bounds
def gamma(k):
    return k * U / (1 - k * U)


def sqrt_fraction(q, digits=60):
    """sqrt of a non-negative Fraction to `digits` decimals (rounded down), as a Fraction."""
    s = 10 ** (2 * digits)
    return Fraction(math.isqrt(q.numerator * s // q.denominator), 10 ** digits)


def exact_stats(rows):
    """The twelve statistics of finite rows [n, >= 2] in exact arithmetic (RMS_R, GEO_R to 60 decimals), and the sums the bounds need."""
    r = _rows2d(rows)
    n = len(r)
    xs, zs = [Fraction(float(v)) for v in r[:, 0]], [Fraction(float(v)) for v in r[:, 1]]
    if n == 0:
        return dict(n=0)
    cx, cz = sum(xs) / n, sum(zs) / n
    dx, dz = [x - cx for x in xs], [z - cz for z in zs]
    mxx, mzz, mxz = sum(d * d for d in dx) / n, sum(d * d for d in dz) / n, sum(a * b for a, b in zip(dx, dz)) / n
    geo2 = max(a * a + b * b for a, b in zip(dx, dz))
    val = [Fraction(n), cx, cz, min(xs), max(xs), min(zs), max(zs), mxx, mzz, mxz, sqrt_fraction(mxx + mzz), sqrt_fraction(geo2)]
    return dict(n=n, val=val, ax=sum(abs(x) for x in xs), az=sum(abs(z) for z in zs), adx=[abs(d) for d in dx], adz=[abs(d) for d in dz])


def stat_bounds(ex):
    """Bound of |computed - exact| for each of the twelve statistics (Fractions; derivations in the module docstring)."""
    n, v = ex["n"], ex["val"]
    ecx, ecz = gamma(n + 1) * ex["ax"] / n, gamma(n + 1) * ex["az"] / n
    g = gamma(n + 3)
    bxx = g * (v[MXX] + ecx * ecx) + ecx * ecx
    bzz = g * (v[MZZ] + ecz * ecz) + ecz * ecz
    s_xz = sum((a + ecx) * (b + ecz) for a, b in zip(ex["adx"], ex["adz"])) / n
    bxz = g * s_xz + ecx * ecz
    s = v[MXX] + v[MZZ]
    d = (bxx + bzz) + U * (s + bxx + bzz)
    up = sqrt_fraction(d) + Fraction(1, 10 ** 59)  # rounded up
    root = sqrt_fraction(s) + sqrt_fraction(max(Fraction(0), s - d))
    move = min(d / root, up) if root > 0 else up
    brms = move + U * (v[RMS_R] + move) + Fraction(1, 10 ** 59)
    h = sqrt_fraction(ecx * ecx + ecz * ecz) + Fraction(1, 10 ** 59)
    bgeo = h + gamma(4) * (v[GEO_R] + h) + Fraction(1, 10 ** 59)
    zero = Fraction(0)
    return [zero, ecx, ecz, zero, zero, zero, zero, bxx, bzz, bxz, brms, bgeo]


def stat_violations(got, rows, ex=None):
    """[(name, got, exact, |error|, bound), ...] of the statistics `got` [12] that miss their bound on `rows` (empty: all inside).  A row set
    without rows must read N = 0 and NaN elsewhere."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (STAT_N,)
    ex = exact_stats(rows) if ex is None else ex
    if ex["n"] == 0:
        ok = got[N] == 0 and np.isnan(got[1:]).all()
        return [] if ok else [("empty", got.tolist(), None, None, None)]
    bad = []
    for k, (e, b) in enumerate(zip(ex["val"], stat_bounds(ex))):
        if not math.isfinite(got[k]):
            bad.append((STAT_NAMES[k], got[k], float(e), math.inf, float(b)))
            continue
        err = abs(Fraction(float(got[k])) - e)
        if err > b:
            bad.append((STAT_NAMES[k], got[k], float(e), float(err), float(b)))
    return bad


def two_pass_sequential(rows):
    """The two-pass formulas in plain sequential float64 (one Python float operation per rounding)."""
    r = _rows2d(rows)
    n = len(r)
    out = np.full(STAT_N, np.nan)
    out[N] = n
    if n == 0:
        return out
    sx = sz = 0.0
    for x, z in r[:, :2].tolist():
        sx += x
        sz += z
    cx, cz = sx / n, sz / n
    mxx = mzz = mxz = geo = 0.0
    for x, z in r[:, :2].tolist():
        dx, dz = x - cx, z - cz
        mxx += dx * dx
        mzz += dz * dz
        mxz += dx * dz
        geo = max(geo, dx * dx + dz * dz)
    mxx, mzz, mxz = mxx / n, mzz / n, mxz / n
    out[1:] = [cx, cz, r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max(), mxx, mzz, mxz, math.sqrt(mxx + mzz), math.sqrt(geo)]
    return out


def one_pass_mxx(rows):
    """MXX by the textbook one-pass form sum x^2 / n - cx^2 in sequential float64: what the engine must NOT do."""
    x = np.asarray(rows, dtype=np.float64)[:, 0].tolist()
    s = s2 = 0.0
    for v in x:
        s += v
        s2 += v * v
    c = s / len(x)
    return (s2 - len(x) * (c * c)) / len(x)


# ------------------------------------------------------------------------------------------------ inputs
def window_rows(n, window, seed, row_cols=2, crafted=True):
    """n rows of row_cols columns: uniform over 1.5 x the window, the leading ones replaced by crafted rows (on each edge, one ulp outside
    each edge, a NaN, +inf, -inf).  Columns past z hold a filler that must not be read as a coordinate."""
    x0, x1, z0, z1 = window
    rng = np.random.default_rng(seed)
    cx, cz, hx, hz = (x0 + x1) / 2, (z0 + z1) / 2, (x1 - x0) / 2, (z1 - z0) / 2
    rows = np.full((n, row_cols), 1e30)
    rows[:, 0] = cx + 1.5 * hx * rng.uniform(-1, 1, n)
    rows[:, 1] = cz + 1.5 * hz * rng.uniform(-1, 1, n)
    if crafted:
        mz = (z0 + z1) / 2
        special = [(x0, mz), (x1, mz), (cx, z0), (cx, z1), (np.nextafter(x0, -np.inf), mz), (np.nextafter(x1, np.inf), mz),
                   (cx, np.nextafter(z0, -np.inf)), (cx, np.nextafter(z1, np.inf)), (x1, z1), (x0, z0), (np.nan, mz), (cx, np.nan),
                   (np.inf, mz), (cx, -np.inf), (np.nextafter(x0, np.inf), mz), (np.nextafter(x1, -np.inf), mz)]
        k = min(n, len(special))
        rows[:k, 0:2] = np.array(special[:k]).reshape(k, 2)
    return rows


def finite_rows(n, seed, row_cols=2, center=(0.3e-3, -0.2e-3), spread=1e-3):
    """n finite rows around `center` (metres), for the statistics."""
    rng = np.random.default_rng(seed)
    rows = np.full((n, row_cols), 1e30)
    rows[:, 0] = center[0] + spread * rng.standard_normal(n)
    rows[:, 1] = center[1] + 0.5 * spread * rng.uniform(-1, 1, n)
    return rows


def offset_spot(n=4000, seed=11):
    """A spot 1e-7 m across, 1e-2 m off centre: the one-pass moment loses ten digits here."""
    return finite_rows(n, seed, center=(1e-2, -1e-2), spread=1e-7)
