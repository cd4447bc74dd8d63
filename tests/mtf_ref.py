"""Helpers of the MTF read-out tests (not a test file): 40-digit evaluations written from the formulas of include/bmo.h "MTF read-out" alone,
and the error bounds of the engine's arithmetic, derived here and not fitted.

Convention: frequencies (fx, fz) in cycles per metre in the detector's local frame,

    T(f) = sum w cis(-2 pi (fx x + fz z)),      MTF(f) = |T(f)| / T(0).

1. geo_otf_exact: every row propagated along its direction to the plane through o_m = origin + offsets[m] axis (exact) with normal e1 x e2
   (exact), as focus_ref.focus_stats_exact does it; x and z there, less the centre (cx_m, cz_m) given as doubles; the phase goes through
   expjpi(-2 (fx ax + fz az)), so no value of pi is rounded.  T is the 40-digit sum rounded once at the end; S = sum proj.

2. otf_exact: T(f) = sum_ij I[i, j] expjpi(-2 (fx xs[i] + fz zs[j])) of an image of doubles, likewise.

3. The bounds.  u = 2^-53, gamma_k = k u / (1 - k u).

   Geometric, each component of T against (1) (geo_bound):  B = (2 pi da + 14 u + (H + 1) u) S + u |T|.
     da, the error of the argument a = fl(fl(fx ax) + fl(fz az)) in cycles:
       the engine's x and z are within E_row = u kappa^2 (12 L + 36 R) of the exact ones (focus_ref, "The statistics");
       ax = fl(x - cx) adds u |ax|: |dax| <= E_row + u |ax|, the same for az;
       the two products and the sum: gamma_2 (|fx ax| + |fz az|);
       da <= (|fx| + |fz|) E_row + 3 u (|fx| AX + |fz| AZ) (1 + 1e-9),   AX = max |ax| + E_row, AZ likewise.
       -2.0 * a is exact; sincospi takes the argument in half turns, so a cycle of argument error is 2 pi radians, each of which moves cis by
       at most one unit in modulus and so in each component.
     14 u: the two sincospi components at the OpenCL FP64 bound of 4 ulp, an ulp of a value in [-1, 1] being at most 2 u: 8 u per
       component, 8 sqrt(2) u = 11.32 u for the complex value; the product fl(proj c) adds u: 12.32 u, stated as 14 u.
     (H + 1) u S: the sum over H rows in any order, gamma_{H-1} sum |term|.     u |T|: the 40-digit value rounded to complex128.

   Transform, each component of T against (2) of the image the same call returned (otf_bound):
       B = (2 pi u max_ij (|fx x_i| + |fz z_j|) + 27 u + 2 n u) sum I (1 + 1e-9) + u |T|
     the arguments fl(fx * x_i) and fl(fz * z_j) are each within u of themselves, in cycles; two sincospi (2 * 11.32 u = 22.63 u); the
     product fl(I cx) (u); the complex product of the row sum with the z factor (2 u): 25.63 u, stated as 27 u (focus_ref.C_TERM); the
     two sequential sums of n terms each, gamma_{n-1} twice: 2 n u.

   MTF (mtf_bound): |T| moves by at most sqrt(2) B.  fl(sqrt(fl(fl(re re) + fl(im im)))) / S^: the squares, their sum, the root and the
   quotient are inside 4 u relative; S^ carries gamma_{H-1} (geometric: H rows; transform: n n samples, gamma_{2n}):
       sqrt(2) B / S + (4 u + gamma) MTF (1 + 1e-9).
"""
import math

import numpy as np

import focus_ref as fr

U = fr.U
C_SINCOSPI = 14.0
C_TRANSFORM = fr.C_TERM


def _ex(mp, a):
    return [mp.mpf(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def _freqs(freqs):
    return np.asarray(freqs, dtype=np.float64).reshape(-1, 2)


# planted mistakes of the exact evaluators (tests/test_mtf_ref.py shows that each misses a known answer by far more than a bound)
MISTAKES = ("pi_for_2pi", "swap_fx_fz", "n_for_s", "cycles_per_mm")


def _phase_args(fq, mistake):
    """(fx, fz, turns): the frequencies as the evaluator uses them and the half turns of expjpi per cycle (2 when right)."""
    fx, fz = float(fq[0]), float(fq[1])
    if mistake == "swap_fx_fz":
        fx, fz = fz, fx
    if mistake == "cycles_per_mm":
        fx, fz = fx * 1e-3, fz * 1e-3
    return fx, fz, (1 if mistake == "pi_for_2pi" else 2)


def local_xz_exact(hits, origin, e1, e2, axis, offsets):
    """[[(x, z) mpf per row] per plane]: the rows propagated exactly to each plane; call it inside mp.workdps(40)."""
    import mpmath as mp

    o, a1, a2, ax = _ex(mp, origin), _ex(mp, e1), _ex(mp, e2), _ex(mp, axis)
    nrm = [a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]]
    rows = [_ex(mp, r) for r in np.asarray(hits, dtype=np.float64).reshape(-1, 9)]
    out = []
    for off in _ex(mp, offsets):
        om = [o[k] + off * ax[k] for k in range(3)]
        plane = []
        for r in rows:
            s = mp.fsum((om[k] - r[k]) * nrm[k] for k in range(3)) / mp.fsum(r[3 + k] * nrm[k] for k in range(3))
            q = [r[k] + s * r[3 + k] for k in range(3)]
            plane.append((mp.fsum((q[k] - om[k]) * a1[k] for k in range(3)), mp.fsum((q[k] - om[k]) * a2[k] for k in range(3))))
        out.append(plane)
    return out


def geo_otf_exact(hits, origin, e1, e2, axis, offsets, freqs, centers=None, mistake=None):
    """(T [M, nf] complex128, S float, scales): the exact geometric transfer function; scales[m] = (max |ax|, max |az|) of plane m."""
    import mpmath as mp

    assert mistake is None or mistake in MISTAKES
    h = np.asarray(hits, dtype=np.float64).reshape(-1, 9)
    fq = _freqs(freqs)
    off = np.asarray(offsets, dtype=np.float64).reshape(-1)
    cen = np.zeros((len(off), 2)) if centers is None else np.asarray(centers, dtype=np.float64).reshape(len(off), 2)
    T = np.zeros((len(off), len(fq)), dtype=np.complex128)
    scales = []
    with mp.workdps(40):
        w = _ex(mp, h[:, 7])
        S = float(len(h)) if mistake == "n_for_s" else float(mp.fsum(w))
        for m, plane in enumerate(local_xz_exact(h, origin, e1, e2, axis, off)):
            cx, cz = mp.mpf(float(cen[m, 0])), mp.mpf(float(cen[m, 1]))
            axz = [(x - cx, z - cz) for x, z in plane]
            scales.append((float(max([abs(a) for a, _ in axz] or [0])), float(max([abs(b) for _, b in axz] or [0]))))
            for q, f in enumerate(fq):
                fx, fz, turns = _phase_args(f, mistake)
                fx, fz = mp.mpf(fx), mp.mpf(fz)
                acc = mp.mpc(0)
                for wi, (a, b) in zip(w, axz):
                    acc += wi * mp.expjpi(-turns * (fx * a + fz * b))
                T[m, q] = complex(acc)
    return T, S, scales


def otf_exact(I, xs, zs, freqs, mistake=None):
    """(T [nf] complex128, sum I): the exact transform of the image I[i, j] of doubles sampled at (xs[i], zs[j])."""
    import mpmath as mp

    assert mistake is None or mistake in MISTAKES
    img = np.asarray(I, dtype=np.float64)
    assert img.shape == (len(xs), len(zs))
    fq = _freqs(freqs)
    T = np.zeros(len(fq), dtype=np.complex128)
    with mp.workdps(40):
        x, z = _ex(mp, xs), _ex(mp, zs)
        v = [[mp.mpf(float(img[i, j])) for j in range(len(z))] for i in range(len(x))]
        total = float(img.size) if mistake == "n_for_s" else float(mp.fsum(mp.fsum(r) for r in v))
        for q, f in enumerate(fq):
            fx, fz, turns = _phase_args(f, mistake)
            fx, fz = mp.mpf(fx), mp.mpf(fz)
            cx = [mp.expjpi(-turns * (fx * a)) for a in x]
            cz = [mp.expjpi(-turns * (fz * b)) for b in z]
            T[q] = complex(mp.fsum(mp.fsum(v[i][j] * cx[i] for i in range(len(x))) * cz[j] for j in range(len(z))))
    return T, total


# ------------------------------------------------------------------------------------------------ the bounds
def geo_bound(n_rows, s, e_row, scale, f, t_abs=0.0):
    """B of the module docstring for one plane and one frequency f = (fx, fz): each component of T.  e_row: focus_ref's E_row of the plane;
    scale: (max |ax|, max |az|) of its rows."""
    fx, fz = abs(float(f[0])), abs(float(f[1]))
    da = (fx + fz) * e_row + 3 * U * (fx * (scale[0] + e_row) + fz * (scale[1] + e_row)) * (1 + 1e-9)
    return (2 * math.pi * da + C_SINCOSPI * U + (n_rows + 1) * U) * s * (1 + 1e-9) + U * t_abs


def e_row(ex):
    """focus_ref's E_row from one plane's dict of focus_ref.focus_stats_exact."""
    return U * ex["kappa"] ** 2 * (12 * ex["L"] + 36 * ex["R"])


def otf_bound(total, xs, zs, f, t_abs=0.0):
    n = max(len(xs), len(zs))
    arg = 2 * math.pi * U * (abs(float(f[0])) * float(np.abs(xs).max()) + abs(float(f[1])) * float(np.abs(zs).max()))
    return (arg + C_TRANSFORM * U + 2 * n * U) * total * (1 + 1e-9) + U * t_abs


def mtf_bound(field_bound, s, mtf, n_terms):
    return math.sqrt(2) * field_bound / s + (4 * U + fr.gamma(n_terms)) * mtf * (1 + 1e-9)


# ------------------------------------------------------------------------------------------------ the Airy scene in numpy
def pupil_rho(rows, e1, e2):
    """RHO of include/bmo.h "Zernike read-out" in plain numpy: the largest distance of a row's direction cosines from their proj-weighted mean."""
    h = np.asarray(rows, dtype=np.float64).reshape(-1, 9)
    u, v, w = h[:, 3:6] @ np.asarray(e1), h[:, 3:6] @ np.asarray(e2), h[:, 7]
    u0, v0 = (w * u).sum() / w.sum(), (w * v).sum() / w.sum()
    return float(np.sqrt(((u - u0) ** 2 + (v - v0) ** 2).max()))


def otf_numpy(I, xs, zs, freqs):
    """(mtf, T) of the image I[i, j] in numpy: the separable transform with np.exp, for the sampling test (accuracy 1e-12, not a yardstick
    of the engine's rounding)."""
    fq = _freqs(freqs)
    cx = np.exp(-2j * np.pi * fq[:, 0:1] * np.asarray(xs)[None, :])
    cz = np.exp(-2j * np.pi * fq[:, 1:2] * np.asarray(zs)[None, :])
    T = np.einsum("fi,ij,fj->f", cx, np.asarray(I, dtype=np.float64), cz)
    return np.abs(T) / float(np.sum(I)), T
