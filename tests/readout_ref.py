"""Helpers of the read-out tests (not a test file).

1. psf_field_exact: the coherent sum of intensity(psf) (PSFDetector.jl:225-232 of the reference) at 40 significant digits,

       p = origin + x e1 + z e2,   l = dot(p - pos_h, dir_h),   F(x, z) = sum_h proj_h cis(k_h (opl_h + l)),

   with every input taken as the exact value of its double.  It is written from that formula alone, not from oracle/bmo_oracle.cpp: exact
   rational-free mpmath arithmetic, no prescribed operation order, and the phase goes through expjpi (cis(phi) = exp(i pi (phi / pi))), so
   it shares neither the oracle's rounding sequence nor a libm with it.  About 8 000 (point, hit) pairs per second: keep a case below
   about 5 * 10^4 pairs.

2. The derived error bounds of the read-outs (u = 2^-53, S = sum_h proj_h):
     oracle - exact   (psf_oracle_bound):  (3 u max_h |phase_h| + 2 H u + 8 u) S
         two roundings in forming phase = k * (opl + l) plus the propagated rounding of l (3 u |phase| of argument error, each radian of
         which moves cis by one unit), the sequential sum (2 H u S covers (H - 1) u S twice over, re and im), libm and the product (8 u).
     engine - oracle  (psf_engine_bound):  (12 + 2 H) u S
         both feed bit-identical phases to sincos.  OpenCL's FP64 bound is 4 ulp per sincos component on the device, glibc gives 1 ulp on the
         host: 5 ulp = 10 u per component, sqrt(2) of it for the modulus and the rounding of proj * c on both sides stay below 12 u proj
         per term; the sequential-sum worst case is (H - 1) u S per side, and the engine's blocked sum is inside it.

3. Restatements of the engine's work splitting (psf_splits, pd_splits and the launches of SplitPlan in csrc/bmo_readout.inc.hpp).  The tests use
   them ONLY to assert that a chosen shape reaches the code path it was chosen for, never to compute an expected value.
"""
import math
import os
import re

import numpy as np

U = 2.0 ** -53
PSF_TILE = 256
READOUT_SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "beamletoptics.jl_amd", "csrc", "bmo_readout.inc.hpp")


def psf_field_exact(hits, origin, e1, e2, xs, zs):
    """F[i, j] at (xs[i], zs[j]) as complex128 (the 40-digit sum rounded once at the end); hits [H, 9] = pos 0-2, dir 3-5, opl 6, proj 7, k 8."""
    import mpmath as mp

    with mp.workdps(40):
        ex = lambda a: [mp.mpf(float(v)) for v in a]  # noqa: E731  (a double is a dyadic rational: mpf(float) is exact)
        o, a1, a2 = ex(origin), ex(e1), ex(e2)
        rows = [ex(r) for r in np.asarray(hits, dtype=np.float64).reshape(-1, 9)]
        out = np.zeros((len(xs), len(zs)), dtype=np.complex128)
        for i, x in enumerate(ex(xs)):
            for j, z in enumerate(ex(zs)):
                p = [o[k] + x * a1[k] + z * a2[k] for k in range(3)]
                acc = mp.mpc(0)
                for r in rows:
                    l = mp.fsum((p[k] - r[k]) * r[3 + k] for k in range(3))
                    acc += r[7] * mp.expjpi(r[8] * (r[6] + l) / mp.pi)
                out[i, j] = complex(acc)
    return out


def psf_max_phase(hits, origin, e1, e2, xs, zs):
    """max over (point, hit) of |k (opl + l)|, in plain doubles (it only scales a bound)."""
    h = np.asarray(hits, dtype=np.float64).reshape(-1, 9)
    if len(h) == 0:
        return 0.0
    o, a1, a2 = (np.asarray(v, dtype=np.float64) for v in (origin, e1, e2))
    p = o[None, None, :] + np.asarray(xs)[:, None, None] * a1[None, None, :] + np.asarray(zs)[None, :, None] * a2[None, None, :]
    l = np.einsum("ijk,hk->ijh", p, h[:, 3:6]) - np.einsum("hk,hk->h", h[:, 0:3], h[:, 3:6])[None, None, :]
    return float(np.abs(h[None, None, :, 8] * (h[None, None, :, 6] + l)).max())


def psf_oracle_bound(hits, max_phase):
    h = np.asarray(hits, dtype=np.float64).reshape(-1, 9)
    return (3 * U * max_phase + 2 * len(h) * U + 8 * U) * float(h[:, 7].sum())


def psf_engine_bound(hits):
    h = np.asarray(hits, dtype=np.float64).reshape(-1, 9)
    return (12 + 2 * len(h)) * U * float(h[:, 7].sum())


def source_psf_tile():
    """PSF_TILE as the engine's source states it."""
    m = re.search(r"constexpr\s+int\s+PSF_TILE\s*=\s*(\d+)\s*;", open(READOUT_SOURCE).read())
    assert m, "PSF_TILE not found in " + READOUT_SOURCE
    return int(m.group(1))


def _cdiv(a, b):
    return (a + b - 1) // b


def psf_splits(n_hits, n_pts):
    """(n_splits, hits_per_split) of bmo_psf_intensity for n_hits rows on n_pts grid points."""
    pt_blocks = _cdiv(n_pts, 256)
    n_splits = _cdiv(4096, pt_blocks)
    n_splits = max(1, min(n_splits, _cdiv(n_hits, PSF_TILE)))
    n_splits = min(n_splits, 65535)
    hps = _cdiv(n_hits, n_splits)
    hps = max(PSF_TILE, _cdiv(hps, PSF_TILE) * PSF_TILE)
    return (_cdiv(n_hits, hps) if n_hits > 0 else 1), hps


def psf_tiles(n_hits, n_pts):
    """LDS tiles (their hit counts) of every split: [[256, 256, 136], ...]."""
    n_splits, hps = psf_splits(n_hits, n_pts)
    out = []
    for s in range(n_splits):
        h0, h1 = s * hps, min((s + 1) * hps, n_hits)
        out.append([min(PSF_TILE, h1 - b) for b in range(h0, h1, PSF_TILE)])
    return out


def pd_splits(n_hits, n_pts):
    """(n_splits, hits_per_split) of bmo_photodetector_field for n_hits > 0 recorded beamlets on n_pts grid points."""
    pt_blocks = _cdiv(n_pts, 256)
    n_splits = max(1, min(_cdiv(2048, pt_blocks), n_hits, 65535))
    hps = _cdiv(n_hits, n_splits)
    return _cdiv(n_hits, hps), hps


def sweep_launches(splits_per_cfg, n_pts):
    """[(c0, nc), ...]: the launches of a sweep read-out (SplitPlan) whose configuration c has splits_per_cfg[c] splits (0: no rows).  A launch
    takes consecutive configurations while their splits fit min(65535, 1 GiB of 16-byte partial sums per point) rows, at most 65535 of
    them; a configuration that alone has more goes alone."""
    cap = max(1, min(65535, (1 << 30) // (n_pts * 16)))
    out, c, K = [], 0, len(splits_per_cfg)
    while c < K:
        c0, rows = c, 0
        while c < K and c - c0 < 65535 and (c == c0 or rows + splits_per_cfg[c] <= cap):
            rows += splits_per_cfg[c]
            c += 1
        out.append((c0, c - c0))
    return out


# ------------------------------------------------------------------------------------------------ the tilted PSF scene
def tilted_psf_case(num_rays):
    """The Airy KAT's lens with an oblique, decentred bundle and a PSFDetector that is rotated about z, x and z again and moved off the axis:
    no component of its e1 / e2 is zero.  Returns (system, detector, bundle)."""
    import bmo_amd as bmo
    import scenes

    mm = 1e-3
    lens = bmo.SphericalLens(100 * mm, math.inf, 1 * mm, 25.4 * mm, lambda lam_: 1.5)
    psfd = bmo.PSFDetector(10 * mm)
    bmo.zrotate3d(psfd, math.radians(5))
    bmo.xrotate3d(psfd, math.radians(8))
    bmo.zrotate3d(psfd, math.radians(-3))
    bmo.translate3d(psfd, [0.4 * mm, 200.13 * mm, -0.3 * mm])
    bundle = scenes.disc_bundle(num_rays, center=[0.2 * mm, -10 * mm, 0.1 * mm], direction=[0.004, 1.0, -0.006], diameter=12 * mm, lam=1e-6, jitter=1e-3)
    return bmo.System([lens, psfd]), psfd, bundle
