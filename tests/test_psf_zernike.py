"""Zernike read-out on the GPU: bmo_psf_zernike against the exact normal equations of the same per-row doubles, inside the derived bounds
of tests/zernike_ref.py (nothing fitted): synthetic rows at the project's scales, planted aberrations and an analytic tilt on a perfect
focus, and a real solve."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import psf_stats_ref as pr
import spot_ref as sr
import zernike_ref as zr
from test_psf_readout import airy_setup
from test_psf_stats import same_bits

pytestmark = pytest.mark.gpu

RAGGED = sr.smallest_ragged_three_splits()
GIVEN_REF = (pr.F_LOCAL[0] + 2e-7, pr.F_LOCAL[1] - 1e-7)
GIVEN_PUPIL = (1e-3, -2e-3, 0.057)  # holds the f/13 square of synthetic_rows: (0.0375 + 0.002) sqrt 2 = 0.0559
U = 2.0 ** -53


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def _resident(rows, pose, **kw):
    """the fit of a copy of the rows in device memory"""
    hip = C.CDLL("libamdhip64.so")
    rows = np.ascontiguousarray(rows)
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(max(rows.nbytes, 8))) == 0
    try:
        assert hip.hipMemcpy(dptr, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return abi.psf_zernike(None, *pose, hits_device_ptr=dptr.value, n_hits=len(rows), want_gram=True, **kw)
    finally:
        hip.hipFree(dptr)


def check_fit(rows, pose, order, ref, pupil, coef, info, gram):
    """Every check of one call that needs no knowledge of the wavefront; returns what the callers reuse (None where the fit was not
    attempted)."""
    n, J = len(rows), zr.n_terms(order)
    assert coef.shape == (J,) and info.shape == (zr.INFO_N,) and gram.shape == ((J + 1) * (J + 2) // 2,)
    if n == 0:
        assert info[zr.N] == 0 and info[zr.STATUS] == 1 and np.isnan(np.delete(info, [zr.N, zr.STATUS])).all()
        assert np.isnan(coef).all() and np.isnan(gram).all()
        return None
    st = abi.psf_stats(rows, *pose, ref=ref)[0]
    assert info[zr.N] == n
    for a, b in ((zr.S, pr.S), (zr.X_REF, pr.X_REF), (zr.Z_REF, pr.Z_REF), (zr.W_MEAN, pr.W_MEAN)):
        assert same_bits(info[a], st[b]), (a, info[a], st[b])
    u, v = zr.cosines(rows, pose[1], pose[2])
    if pupil is None:
        ex = pr.exact_stats(u, v, u, rows[:, 7])
        _, e_u, e_v, _, _, _ = pr.sum_bounds(ex)
        assert abs(Fraction(float(info[zr.U0])) - ex["cx"]) <= e_u and abs(Fraction(float(info[zr.V0])) - ex["cz"]) <= e_v
        du, dv = u - info[zr.U0], v - info[zr.V0]
        assert same_bits(info[zr.RHO], np.sqrt((du * du + dv * dv).max()))
    else:
        assert same_bits(info[[zr.U0, zr.V0, zr.RHO]], pupil)
    usable = n >= J and info[zr.RHO] != 0 and np.isfinite(info[zr.RHO])
    if not usable:
        assert info[zr.STATUS] == 1 and np.isnan(coef).all() and np.isnan(info[[zr.FIT_RMS, zr.E_LO, zr.E_HI]]).all()
    if info[zr.RHO] == 0:  # one row and its own pupil: no coordinates
        return None
    proj, B, x, y = zr.columns(rows, pose, info, order)
    assert info[zr.N_OUT] == int(((x * x + y * y) > 1.0).sum())
    G, A = zr.exact_gram(proj, B)
    assert zr.gram_violations(gram, G, A, n) == []
    if not usable:
        return None
    want, status, L = zr.cholesky_solve(gram, J)
    assert info[zr.STATUS] == status == 0
    assert same_bits(coef, want)
    E = zr.residual(B, coef)
    assert same_bits(info[zr.E_LO], E.min()) and same_bits(info[zr.E_HI], E.max())
    rms, b_rms = zr.fit_rms_exact(proj, E)
    assert abs(Fraction(float(info[zr.FIT_RMS])) - rms) <= b_rms, (info[zr.FIT_RMS], float(rms), float(b_rms))
    out = dict(proj=proj, B=B, G=G, x=x, y=y, E=E, b_rms=float(b_rms))
    c, bound, Ginv = zr.coef_bounds(gram, G, J, coef, L)
    assert zr.coef_violations(coef, c, bound) == []
    out.update(c=c, bound=[float(b) for b in bound], Ginv=Ginv)
    return out


COUNTS = [0, 1, 64, 65, 255, 256, 257, 300, RAGGED, 5000]
CASES = [(n, o) for o in (2, 4, 6) for n in sorted(set(COUNTS + [zr.n_terms(o) - 1])) if o == 2 or n <= 300]


@pytest.mark.parametrize("n,order", CASES)
def test_synthetic_rows_inside_every_bound(pose, n, order):
    """Exact checks at orders 4 and 6 stay at n <= 300, the larger counts run at order 2 (each case a few seconds).  Every check, the rational
    inverse included, runs for all four combinations of ref and pupil, computed and given."""
    if n == RAGGED:
        ns, per = sr.spot_splits(n)
        assert ns >= 3 and n % per
    rows = pr.synthetic_rows(n, 100 + n, pose)
    J = zr.n_terms(order)
    for ref in (None, GIVEN_REF):
        for pupil in (None, GIVEN_PUPIL):
            coef, info, gram, ms = abi.psf_zernike(rows, *pose, order=order, ref=ref, pupil=pupil, want_gram=True)
            c2, i2, g2, _ = _resident(rows, pose, order=order, ref=ref, pupil=pupil)
            assert same_bits(coef, c2) and same_bits(info, i2) and same_bits(gram, g2), (ref, pupil)
            assert same_bits(abi.psf_zernike(rows, *pose, order=order, ref=ref, pupil=pupil)[0], coef)  # without the gram
            r = check_fit(rows, pose, order, ref, pupil, coef, info, gram)
            print("n = %d, order %d, ref %s, pupil %s: STATUS %d  RHO %.6g  N_OUT %d  FIT_RMS %.4g  max |c| %.4g  %s"
                  % (n, order, ref, pupil, info[zr.STATUS], info[zr.RHO], 0 if n == 0 else info[zr.N_OUT], info[zr.FIT_RMS],
                     np.abs(coef).max() if r else math.nan, "max bound %.3g" % max(r["bound"]) if r else ""))
            if n < J:
                assert info[zr.STATUS] == 1 and np.isnan(coef).all()
            else:
                assert r is not None and info[zr.STATUS] == 0 and ms > 0
                # the given pupil holds every row; about the computed RHO only the outermost row can round to t = 1 + a few u
                assert info[zr.N_OUT] == 0 if pupil is not None else info[zr.N_OUT] <= 1
                if n >= 64:  # non-vacuity
                    assert max(r["bound"]) < 1e-6 * np.abs(coef).max(), (max(r["bound"]), np.abs(coef).max())


def test_rows_outside_a_small_pupil_are_counted_and_fitted(pose):
    rows = pr.synthetic_rows(300, 5, pose)
    pupil = (0.0, 0.0, 0.04)
    coef, info, gram, _ = abi.psf_zernike(rows, *pose, order=2, pupil=pupil, want_gram=True)
    r = check_fit(rows, pose, 2, None, pupil, coef, info, gram)
    assert 0 < info[zr.N_OUT] < 300 and r is not None and info[zr.STATUS] == 0


def _planted(order):
    """coefficients in metres by (n, m): tilt, defocus, astigmatism, coma, spherical, secondary spherical, 5 - 50 nm"""
    a = np.zeros(zr.n_terms(order))
    for (n, m), val in (((1, 1), 50e-9), ((2, 0), -30e-9), ((2, 2), 12e-9), ((3, -1), 8e-9), ((4, 0), 20e-9), ((6, 0), 5e-9)):
        if n <= order:
            a[zr.term_index(n, m)] = val
    return a


@pytest.mark.parametrize("n,order", [(300, 6), (5000, 2), (257, 4)])
def test_planted_aberrations_are_recovered(pose, n, order):
    """focus_rows is a perfect focus: W_h = R within focus_row_error.  delta_h = sum a_j Z_j(x_h, y_h) is added to the opl column at the
    (x_h, y_h) of an explicit pupil, so the engine evaluates the same Z_j doubles.  The new opl = fl(opl + delta) and W = fl(opl + l) round at
    u (R + |delta|) each (the latter was u R in focus_row_error): E = focus_row_error + 2 u R covers both; the float evaluation of delta_h
    (2 J roundings) and the rounding of D_h = fl(W_h - W_MEAN) add the E_small below.  W_h - W_MEAN = const + sum a_j Z_j + e_h with
    |e_h| <= E, and Z_0 = 1 takes the constant, so the exact least-squares c_j = a_j + (G^-1 sum proj z_h e_h)_j for j >= 1:
        |c^_j - a_j| <= E sum_h proj_h |(G^-1 z_h)_j| + the coefficient bound.
    The weighted RMS residual of the exact fit is at most that of e (E); the computed coefficients add sum_j bound_j sqrt(G_jj / S)."""
    rows, f = pr.focus_rows(n, 31 + n, pose)
    u, v = zr.cosines(rows, pose[1], pose[2])
    pupil = (2e-3, -1e-3, 0.06)
    x, y = zr.pupil_xy(u, v, *pupil)
    a = _planted(order)
    J = len(a)
    Z = zr.basis(x, y, order)
    rows[:, 6] += np.tensordot(a, Z, axes=1)
    coef, info, gram, _ = abi.psf_zernike(rows, *pose, order=order, ref=pr.F_LOCAL, pupil=pupil, want_gram=True)
    r = check_fit(rows, pose, order, pr.F_LOCAL, pupil, coef, info, gram)
    assert same_bits(r["x"], x) and same_bits(r["y"], y) and info[zr.N_OUT] == 0
    size = (np.abs(a)[:, None] * np.abs(Z)).sum(axis=0).max()
    E = pr.focus_row_error(f) + 2 * U * pr.FOCUS_R + (2 * J + 2) * U * (size + np.abs(r["B"][J]).max())
    img = zr.image_of_row_error(r["Ginv"], r["proj"], r["B"], J)
    err = np.abs(coef - a)
    print("n = %d, order %d: E %.3g  image of E %.3g .. %.3g  coefficient bound max %.3g  |c - a| max (j >= 1) %.3g  FIT_RMS %.3g"
          % (n, order, E, (E * img[1:]).min(), (E * img[1:]).max(), max(r["bound"]), err[1:].max(), info[zr.FIT_RMS]))
    for j in range(1, J):
        assert err[j] <= E * img[j] + r["bound"][j], (j, err[j], E * img[j], r["bound"][j])
    S = float(sum(pr._fr(r["proj"])))
    rms_z = [math.sqrt(float(r["G"][zr.packed(j, j)]) / S) * (1 + 4 * U) for j in range(J)]
    assert info[zr.FIT_RMS] <= E + sum(b * z for b, z in zip(r["bound"], rms_z)) + r["b_rms"]
    assert (E * img[1:]).max() + max(r["bound"]) < 1e-3 * 5e-9  # the planted 5 nm is resolved a thousand times over


def test_a_moved_reference_point_is_a_pure_tilt(pose):
    """focus_rows read at p' = ref_point(F_LOCAL + (dx, 0)): l'_h = (p' - hit_h) . dir_h = (f - hit_h) . dir_h + (p' - f) . dir_h, and
    p' - f = dx e1 + eta, where eta collects the roundings of the two ref_point evaluations: three operations each, so
    |eta|_1 <= 7 u |f|_1 (dx = 20 um adds less than 7 u dx).  dx (e1 . dir_h) = dx u_h up to the rounding of u_h (gamma_3 dx), and
    u_h = U0 + RHO x_h up to the two roundings of x_h (2 u RHO dx); the differences p' - hit and their dot product are now of size
    s + dx instead of s (4 u dx more).  So  W_h = const + (dx RHO / 2) Z_1^1(x_h, y_h) + e_h,  Z_1^1 = 2 x,  |e_h| <= E with
        E = focus_row_error + u (7 |f|_1 + 16 dx),
    plus the rounding of D_h as in the planted test.  (W grows with +dx u_h: l is the path from the hit to p along dir.)  Hence
    c(Z_1^1) = dx RHO / 2 and every other term of j >= 1 is zero, each within E's image + the coefficient bound; FIT_RMS falls to E while
    the W_RMS of bmo_psf_stats at the same point is above 1e-7.  This E is deliberately larger than the focus_row_error + 2 u R that goes
    with a reference point at f itself: the u (7 |f|_1 + 16 dx) is the derived price of evaluating ref_point a second time at the moved
    point, and without it the bound would not cover the rounding of p'."""
    n, order, dx = 300, 4, 20e-6
    rows, f = pr.focus_rows(n, 21, pose)
    moved = (pr.F_LOCAL[0] + dx, pr.F_LOCAL[1])
    coef, info, gram, _ = abi.psf_zernike(rows, *pose, order=order, ref=moved, want_gram=True)
    r = check_fit(rows, pose, order, moved, None, coef, info, gram)
    J = zr.n_terms(order)
    dx_true = float(Fraction(moved[0]) - Fraction(pr.F_LOCAL[0]))
    E = pr.focus_row_error(f) + U * (7 * float(np.abs(f).sum()) + 16 * dx) + 4 * U * np.abs(r["B"][J]).max()
    img = zr.image_of_row_error(r["Ginv"], r["proj"], r["B"], J)
    want = np.zeros(J)
    want[zr.term_index(1, 1)] = dx_true * info[zr.RHO] / 2
    err = np.abs(coef - want)
    print("tilt %.6g m (wanted %.6g), E %.3g, image %.3g .. %.3g, other terms max %.3g, FIT_RMS %.3g"
          % (coef[2], want[2], E, (E * img[1:]).min(), (E * img[1:]).max(), np.abs(np.delete(coef, [0, 2])).max(), info[zr.FIT_RMS]))
    for j in range(1, J):
        assert err[j] <= E * img[j] + r["bound"][j] + U * abs(want[j]), (j, coef[j], want[j], E * img[j], r["bound"][j])
    S = float(sum(pr._fr(r["proj"])))
    rms_z = [math.sqrt(float(r["G"][zr.packed(j, j)]) / S) * (1 + 4 * U) for j in range(J)]
    assert info[zr.FIT_RMS] <= E + sum(b * z for b, z in zip(r["bound"], rms_z)) + r["b_rms"]
    assert abi.psf_stats(rows, *pose, ref=moved)[0][pr.W_RMS] > 1e-7 > 1e6 * info[zr.FIT_RMS]


@pytest.fixture(scope="module")
def airy_rows():
    system, cs, psfd, lam, D = airy_setup(num_rays=1000)
    bmo.solve_system(system, cs)
    assert len(psfd.data) == 1000
    o = np.asarray(psfd.orientation(), dtype=np.float64)
    return psfd, psfd.data.copy(), (np.asarray(psfd.position(), dtype=np.float64), o[:, 0].copy(), o[:, 2].copy())


def test_real_solve(airy_rows):
    """The Airy scene's detector stands 0.13 mm inside the focus of a spherical lens: defocus and spherical aberration (Z_2^0, Z_4^0) are
    the two largest terms of n >= 2, and the fit takes most of the wavefront error."""
    psfd, rows, pose = airy_rows
    coef, info, gram, _ = abi.psf_zernike(rows, *pose, order=4, want_gram=True)
    check_fit(rows, pose, 4, None, None, coef, info, gram)
    c1, i1 = psfd.zernike()
    assert same_bits(c1, coef) and same_bits(i1, info)
    c6, i6 = psfd.zernike(order=6, ref=(1e-6, 0.0), pupil=(0.0, 0.0, 0.05))
    assert same_bits(c6, abi.psf_zernike(rows, *pose, order=6, ref=(1e-6, 0.0), pupil=(0.0, 0.0, 0.05))[0]) and i6[zr.STATUS] == 0
    st = abi.psf_stats(rows, *pose)[0]
    terms = zr.terms(4)
    print("airy: W_RMS %.4g  FIT_RMS %.4g  RHO %.5g  " % (st[pr.W_RMS], info[zr.FIT_RMS], info[zr.RHO])
          + "  ".join("Z(%d,%d) %.3g" % (n, m, c) for (n, m), c in zip(terms, coef)))
    assert info[zr.STATUS] == 0 and info[zr.FIT_RMS] < st[pr.W_RMS]
    high = sorted((j for j, (n, m) in enumerate(terms) if n >= 2), key=lambda j: -abs(coef[j]))
    assert set(high[:2]) == {zr.term_index(2, 0), zr.term_index(4, 0)}
    surf = bmo.components.zernike_surface(coef, 33, 4)
    assert surf.shape == (33, 33) and np.isnan(surf[0, 0]) and np.isfinite(surf[16, 16])


def test_engine_solution_reads_resident_rows(airy_rows):
    psfd, rows, pose = airy_rows
    want_c, want_i, _, _ = abi.psf_zernike(rows, *pose, order=4)
    system, cs, psfd2, lam, D = airy_setup(num_rays=1000)
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    pos, ori = np.asarray(psfd2.position(), dtype=np.float64), np.asarray(psfd2.orientation(), dtype=np.float64)
    for record in (True, False):
        res = eng.trace_device(dev, 100, record_segments=record)
        sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
        try:
            coef, info = sol.psf_zernike(0, pos, ori)
            assert same_bits(coef, want_c) and same_bits(info, want_i), record
            assert sol.readout_ms > 0
            c3, i3 = sol.psf_zernike(0, pos, ori, order=3, ref=(0.0, 1e-6), pupil=(0.0, 0.0, 0.05))
            w3 = abi.psf_zernike(rows, *pose, order=3, ref=(0.0, 1e-6), pupil=(0.0, 0.0, 0.05))
            assert same_bits(c3, w3[0]) and same_bits(i3, w3[1])
        finally:
            sol.handle = None  # the engine frees the result
            eng.free_result(res)
    eng.free_batch(dev)
    eng.close()
