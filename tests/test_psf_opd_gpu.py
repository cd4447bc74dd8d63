"""OPD map read-out on the GPU: bmo_psf_opd_map against the numpy restatement of tests/opd_ref.py, exactly: counts, the integer sums and
every integer info column are equal, opd and weight bit for bit.  Bin-edge decisions need no margin: the engine and the restatement
evaluate the same FP64 expressions on the same doubles (the X_REF .. W_MEAN the call returned), and integer sums have no order.  Then the
exact per-bin means inside the derived bound, planted aberrations on a perfect focus, the statuses, and a real solve."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import opd_ref as od
import psf_stats_ref as pr
import spot_ref as sr
import zernike_ref as zr
from test_psf_readout import airy_setup
from test_psf_stats import same_bits
from test_psf_zernike import _planted, check_fit

pytestmark = pytest.mark.gpu

RAGGED = sr.smallest_ragged_three_splits()
GIVEN_REF = (pr.F_LOCAL[0] + 2e-7, pr.F_LOCAL[1] - 1e-7)
GIVEN_PUPIL = (1e-3, -2e-3, 0.057)
U = 2.0 ** -53
COUNTS = [0, 1, 64, 65, 255, 256, 257, 300, RAGGED, 5000]
# n = 1: every lane of every wave on one bin; 7: bins and the 256-row tiles disagree; 64: the last map in LDS (64 * 64 = OPD_LDS_BINS, more
# dynamic LDS than a launch gets unasked); 65: the first in global memory
BINS = [1, 2, 7, 64]
EDGE = [65]
assert BINS[-1] ** 2 <= od.LDS_BINS < EDGE[0] ** 2


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def _resident(rows, pose, **kw):
    """the map of a copy of the rows in device memory"""
    hip = C.CDLL("libamdhip64.so")
    rows = np.ascontiguousarray(rows)
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(max(rows.nbytes, 8))) == 0
    try:
        assert hip.hipMemcpy(dptr, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return abi.psf_opd_map(None, *pose, hits_device_ptr=dptr.value, n_hits=len(rows), want_raw=True, **kw)
    finally:
        hip.hipFree(dptr)


def flat(a, n):
    """[n, n, ...] indexed [i, j] -> flat with bin (i, j) at i + n j"""
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape(n * n, *a.shape[2:])


def check_map(rows, pose, n, order, coef, got, exact=True):
    """Every output of one call against the restatement; returns (R, proj, E) or None where nothing was binned.  exact: E_RMS against the
    exact root as well (Fractions: a tenth of a second at 5 000 rows)."""
    opd, weight, count, info, raw, _ = got
    N = len(rows)
    assert opd.shape == weight.shape == count.shape == (n, n) and raw.shape == (n, n, 2) and info.shape == (od.INFO_N,)
    assert count.dtype == np.int64 and raw.dtype == np.int64
    if N == 0:
        assert info[od.N] == 0 and info[od.STATUS] == 1 and np.isnan(np.delete(info, [od.N, od.STATUS])).all()
        assert np.isnan(opd).all() and np.isnan(weight).all() and not count.any() and not raw.any()
        return None
    assert info[od.N] == N
    if info[od.RHO] == 0 or not np.isfinite(info[od.RHO]):
        assert info[od.STATUS] == 1 and np.isnan(opd).all() and np.isnan(weight).all() and not count.any() and not raw.any()
        assert info[od.N_OUTSIDE] == N and info[od.N_FILLED] == 0
        assert np.isnan(info[[od.E_RMS, od.E_LO, od.E_HI, od.SH_Q, od.SH_P, od.MAP_LO, od.MAP_HI]]).all()
        return None
    proj, E, x, y = od.rows_of(rows, pose, info, order, coef)
    R = od.restate(proj, E, x, y, n)
    for col in INT_COLS:
        assert info[col] == R[col] or (math.isnan(info[col]) and math.isnan(R[col])), (col, info[col], R[col])
    assert np.array_equal(flat(count, n), R["count"]) and np.array_equal(flat(raw, n), R["raw"])
    assert int(count.sum()) + int(info[od.N_OUTSIDE]) == N
    assert same_bits(flat(opd, n), R["opd"]) and same_bits(flat(weight, n), R["weight"])
    assert same_bits(info[od.MAP_LO], R[od.MAP_LO]) and same_bits(info[od.MAP_HI], R[od.MAP_HI])
    if R[od.STATUS] == 0:
        assert same_bits(info[od.E_LO], E.min()) and same_bits(info[od.E_HI], E.max())
        if exact:
            rms, b_rms = zr.fit_rms_exact(proj, E)
            assert abs(Fraction(float(info[od.E_RMS])) - rms) <= b_rms
    return R, proj, E


INT_COLS = (od.STATUS, od.N_OUT, od.N_OUTSIDE, od.N_BAD, od.N_FILLED, od.SH_Q, od.SH_P)


@pytest.fixture(scope="module")
def fits(pose):
    """rows and one Zernike fit per row count, computed once: (rows, coef, info) at order 2 with computed ref and pupil"""
    out = {}
    for n_rows in COUNTS:
        rows = pr.synthetic_rows(n_rows, 100 + n_rows, pose)
        coef, info, _, _ = abi.psf_zernike(rows, *pose, order=2)
        out[n_rows] = (rows, coef, info)
    return out


@pytest.mark.parametrize("n_rows", COUNTS)
def test_synthetic_rows_equal_the_restatement(pose, fits, n_rows):
    """Every bin count of BINS (and the first above the LDS budget at 300 and 5 000 rows), ref and pupil computed and given; resident rows equal
    host rows bit for bit.  With coef, ref and pupil of the Zernike fit of the same rows, E_RMS, E_LO, E_HI and N_OUT are that fit's bit for bit
    and S, X_REF, Z_REF, W_MEAN those of bmo_psf_stats."""
    if n_rows == RAGGED:
        ns, per = sr.spot_splits(n_rows)
        assert ns >= 3 and n_rows % per
    rows, zc, zi = fits[n_rows]
    solved = n_rows > 0 and zi[zr.STATUS] == 0
    for n in BINS + (EDGE if n_rows in (300, 5000) else []):
        for ref, pupil, order, coef in ((None, None, 0, None), (GIVEN_REF, GIVEN_PUPIL, 1, np.array([2e-9, -1e-9, 3e-9])),
                                        (None, GIVEN_PUPIL, 2, zc if solved else np.zeros(6))):
            kw = dict(n=n, order=order, coef=coef, ref=ref, pupil=pupil)
            got = abi.psf_opd_map(rows, *pose, want_raw=True, **kw)
            res = _resident(rows, pose, **kw)
            for a, b in zip(got[:5], res[:5]):
                assert same_bits(a.astype(np.float64), b.astype(np.float64)) and np.array_equal(a, b, equal_nan=True), kw
            exact = n == 7 or (n == 65 and order == 0)  # the Fraction side once per path (LDS, global memory), the equalities every time
            r = check_map(rows, pose, n, order, coef, got, exact=exact)
            info = got[3]
            if n_rows == 1 and pupil is None:
                assert info[od.STATUS] == 1 and info[od.RHO] == 0  # one row is its own pupil
            elif n_rows > 0:
                assert r is not None and info[od.STATUS] == 0 and got[5] > 0
                if exact:
                    bad, worst, ex = od.map_violations(r[0]["opd"], r[0], r[1], r[2], n)
                    assert bad == []
                    if n_rows == 5000 and order == 0:  # non-vacuity
                        assert float(worst) < 1e-6 * np.nanmax(np.abs(got[0]))
            without_raw = abi.psf_opd_map(rows, *pose, **kw)
            assert without_raw[4] is None and same_bits(without_raw[0], got[0]) and np.array_equal(without_raw[2], got[2])
        if n_rows > 0:
            st = abi.psf_stats(rows, *pose)[0]
            got = abi.psf_opd_map(rows, *pose, n=n, order=2, coef=np.where(np.isfinite(zc), zc, 0.0), ref=zi[[zr.X_REF, zr.Z_REF]],
                                  pupil=zi[[zr.U0, zr.V0, zr.RHO]] if zi[zr.RHO] > 0 else None, want_raw=True)
            info = got[3]
            for a, b in ((od.S, pr.S), (od.X_REF, pr.X_REF), (od.Z_REF, pr.Z_REF), (od.W_MEAN, pr.W_MEAN)):
                assert same_bits(info[a], st[b]), (a, info[a], st[b])
            assert same_bits(info[:od.E_RMS][2:], zi[:zr.FIT_RMS][2:])
            if solved:
                assert same_bits(info[[od.E_RMS, od.E_LO, od.E_HI, od.N_OUT]], zi[[zr.FIT_RMS, zr.E_LO, zr.E_HI, zr.N_OUT]]), (info, zi)
                check_map(rows, pose, n, 2, zc, got, exact=False)
    print("%d rows: fit STATUS %s" % (n_rows, zi[zr.STATUS]))


def test_rows_outside_a_small_pupil_are_counted(pose):
    """(0, 0, 0.04) cuts the corners of the f/13 square of synthetic_rows (half-side 0.0375, corner radius 0.053): rows with t > 1 that lie
    inside the pupil square are binned and counted in N_OUT.  (0, 0, 0.03) also leaves rows outside the square: 0 < N_OUTSIDE < N, and every
    row outside the square is outside the disc: N_OUT >= N_OUTSIDE."""
    rows = pr.synthetic_rows(300, 5, pose)
    for rho in (0.04, 0.03):
        got = abi.psf_opd_map(rows, *pose, n=7, pupil=(0.0, 0.0, rho), want_raw=True)
        r = check_map(rows, pose, 7, 0, None, got)
        info = got[3]
        print("RHO %.2f: N_OUT %d  N_OUTSIDE %d  filled %d" % (rho, info[od.N_OUT], info[od.N_OUTSIDE], info[od.N_FILLED]))
        assert r is not None and info[od.STATUS] == 0
        assert int(got[2].sum()) + info[od.N_OUTSIDE] == 300 and 0 < info[od.N_OUT] < 300 and info[od.N_OUT] >= info[od.N_OUTSIDE]
        if rho == 0.03:
            assert 0 < info[od.N_OUTSIDE] < 300


@pytest.mark.parametrize("n_rows,order", [(300, 6), (5000, 2)])
def test_planted_aberrations_are_mapped(pose, n_rows, order):
    """focus_rows is a perfect focus, W_h = R within focus_row_error; delta_h = sum a_j Z_j(x_h, y_h) (the doubles, taken as the planted
    surface) is added to the opl column as test_psf_zernike.test_planted_aberrations_are_recovered does it: W_h = R + delta_h + e_h with
    |e_h| <= E_row = focus_row_error + 2 u R + 2 u |delta|max.
    Nothing removed: E_h = fl(W_h - W_MEAN) = delta_h + (R - W_MEAN) + e_h within u |D|max more, W_MEAN the double the call returned, so
        opd_b = mean_b(delta) + (R - W_MEAN)  within  E_row + u |D|max + the map bound of opd_ref          (means exact, in Fractions).
    remove = "fit": E_h = D_h - F_h with the computed coefficients c^.  D_h = const + sum a_j Z_j + e_h, the exact least-squares solution is
    c_0 = const + a_0 + (G^-1 sum proj z e)_0 and c_j = a_j + (...)_j, so |c^_j - (a_j [+ const])| <= E_lsq img_j + bound_j for every j, E_lsq = E_row + u |D|max
    (image_of_row_error and coef_bounds of zernike_ref), and
        |E_h| <= E_lsq + sum_j (E_lsq img_j + bound_j) |Z_j(h)| + (2 J + 2) u (sum_j |c^_j Z_j| + |D|)max       (the evaluation of F_h, E_h);
    a bin's mean is at most the largest |E_h|, plus the map bound."""
    rows, f = pr.focus_rows(n_rows, 31 + n_rows, pose)
    u, v = zr.cosines(rows, pose[1], pose[2])
    pupil = (2e-3, -1e-3, 0.06)
    x, y = zr.pupil_xy(u, v, *pupil)
    a = _planted(order)
    J = len(a)
    Z = zr.basis(x, y, order)
    delta = np.tensordot(a, Z, axes=1)
    rows[:, 6] += delta
    n = 7
    got = abi.psf_opd_map(rows, *pose, n=n, ref=pr.F_LOCAL, pupil=pupil, want_raw=True)
    R, proj, E = check_map(rows, pose, n, 0, None, got)
    info = got[3]
    assert info[od.STATUS] == 0 and info[od.N_OUTSIDE] == 0 and info[od.N_OUT] == 0
    bad, map_bound, _ = od.map_violations(R["opd"], R, proj, E, n)
    assert bad == []
    e_row = pr.focus_row_error(f) + 2 * U * pr.FOCUS_R + 2 * U * np.abs(delta).max()
    e_tot = e_row + U * np.abs(E).max() + float(map_bound)
    shift = Fraction(pr.FOCUS_R) - Fraction(float(info[od.W_MEAN]))
    means = od.exact_means(proj, delta, R["key"], n)
    worst = 0.0
    for k, (m, _, _) in means.items():
        err = abs(Fraction(float(R["opd"][k])) - (m + shift))
        worst = max(worst, float(err))
        assert err <= e_tot, (k, float(err), e_tot)
    # the fit removed
    coef, zi, gram, _ = abi.psf_zernike(rows, *pose, order=order, ref=pr.F_LOCAL, pupil=pupil, want_gram=True)
    r = check_fit(rows, pose, order, pr.F_LOCAL, pupil, coef, zi, gram)
    fit = abi.psf_opd_map(rows, *pose, n=n, order=order, coef=coef, ref=zi[[zr.X_REF, zr.Z_REF]], pupil=zi[[zr.U0, zr.V0, zr.RHO]], want_raw=True)
    R2, proj2, E2 = check_map(rows, pose, n, order, coef, fit)
    assert same_bits(fit[3][[od.E_RMS, od.E_LO, od.E_HI, od.N_OUT]], zi[[zr.FIT_RMS, zr.E_LO, zr.E_HI, zr.N_OUT]])
    bad2, map_bound2, _ = od.map_violations(R2["opd"], R2, proj2, E2, n)
    assert bad2 == []
    img = zr.image_of_row_error(r["Ginv"], r["proj"], r["B"], J)
    size = (np.abs(coef)[:, None] * np.abs(Z)).sum(axis=0) + np.abs(r["B"][J])
    e_lsq = e_row + U * np.abs(r["B"][J]).max()  # with the rounding of D_h
    per_row = e_lsq + ((e_lsq * img + np.array(r["bound"]))[:, None] * np.abs(Z)).sum(axis=0) + (2 * J + 2) * U * size
    e_fit = per_row.max() + float(map_bound2)
    print("%d rows, order %d: planted map within %.3g (bound %.3g), residual map max %.3g (bound %.3g), map bounds %.3g / %.3g"
          % (n_rows, order, worst, e_tot, np.nanmax(np.abs(fit[0])), e_fit, float(map_bound), float(map_bound2)))
    assert np.nanmax(np.abs(fit[0])) <= e_fit
    assert e_tot < 1e-3 * 5e-9 and e_fit < 1e-3 * 5e-9  # the planted 5 nm is resolved a thousand times over
    # the Python layer: remove = "fit" is this map, "none" the first
    out = bmo.components.psf_opd_map(lambda od_, rf, q: abi.psf_zernike(rows, *pose, order=od_, ref=rf, pupil=q)[:2],
                                     lambda od_, cf, rf, q: abi.psf_opd_map(rows, *pose, n=n, order=od_, coef=cf, ref=rf, pupil=q)[:4],
                                     n=n, order=order, remove="fit", ref=pr.F_LOCAL, pupil=pupil)
    assert same_bits(out[0], fit[0]) and same_bits(out[4], coef)


def test_status_1_and_2(pose):
    rows = pr.synthetic_rows(300, 9, pose)
    check_map(rows[:0], pose, 4, 0, None, abi.psf_opd_map(rows[:0], *pose, n=4, want_raw=True))
    got = abi.psf_opd_map(rows[:1], *pose, n=4, want_raw=True)
    check_map(rows[:1], pose, 4, 0, None, got)
    assert got[3][od.STATUS] == 1 and got[3][od.N] == 1
    want = abi.psf_opd_map(rows, *pose, n=4, pupil=GIVEN_PUPIL)[2]
    for col, value in ((7, math.nan), (6, math.inf)):
        bad = rows.copy()
        bad[17, col] = value
        opd, weight, count, info, raw, _ = abi.psf_opd_map(bad, *pose, n=4, pupil=GIVEN_PUPIL, want_raw=True)
        assert info[od.STATUS] == 2 and info[od.N_BAD] >= 1 and info[od.N] == 300
        assert np.isnan(opd).all() and np.isnan(weight).all() and not raw.any()
        assert np.array_equal(count, want) and int(count.sum()) + info[od.N_OUTSIDE] == 300 and info[od.N_FILLED] == int((count > 0).sum())
        assert np.isnan(info[[od.SH_Q, od.SH_P, od.MAP_LO, od.MAP_HI]]).all()
        if col == 7:
            assert info[od.N_BAD] >= 1
        else:
            assert info[od.N_BAD] == 300  # W_MEAN is not finite: no row has a finite residual


@pytest.fixture(scope="module")
def airy_rows():
    system, cs, psfd, lam, D = airy_setup(num_rays=1000)
    bmo.solve_system(system, cs)
    assert len(psfd.data) == 1000
    o = np.asarray(psfd.orientation(), dtype=np.float64)
    return psfd, psfd.data.copy(), (np.asarray(psfd.position(), dtype=np.float64), o[:, 0].copy(), o[:, 2].copy())


def test_real_solve(airy_rows):
    """The Airy scene's detector stands 0.13 mm inside the focus: with the defocus term removed as well the map is flatter than with tilt alone."""
    psfd, rows, pose = airy_rows
    n = 16
    tilt = psfd.opd_map(n=n)
    coef, zi, _, _ = abi.psf_zernike(rows, *pose, order=4)
    cf = coef.copy()
    cf[3:] = 0.0
    want = abi.psf_opd_map(rows, *pose, n=n, order=4, coef=cf, ref=zi[[zr.X_REF, zr.Z_REF]], pupil=zi[[zr.U0, zr.V0, zr.RHO]], want_raw=True)
    check_map(rows, pose, n, 4, cf, want)
    assert same_bits(tilt[0], want[0]) and same_bits(tilt[1], want[1]) and np.array_equal(tilt[2], want[2]) and same_bits(tilt[3], want[3])
    assert same_bits(tilt[4], cf)
    defocus = psfd.opd_map(n=n, remove="defocus")
    none = psfd.opd_map(n=n, remove="none")
    pv = lambda o: o[3][od.MAP_HI] - o[3][od.MAP_LO]  # noqa: E731
    print("airy: peak to valley of the map  none %.4g  tilt %.4g  defocus %.4g  fit %.4g m; %d of %d bins filled"
          % (pv(none), pv(tilt), pv(defocus), pv(psfd.opd_map(n=n, remove="fit")), tilt[3][od.N_FILLED], n * n))
    assert tilt[3][od.STATUS] == 0 and pv(defocus) < pv(tilt)
    us, vs = bmo.components.opd_axes(tilt[3], n)
    assert us.shape == (n,) and abs(us[0] - (zi[zr.U0] - zi[zr.RHO] * (1 - 1 / n))) < 1e-15


def test_engine_solution_reads_resident_rows(airy_rows):
    psfd, rows, pose = airy_rows
    want = psfd.opd_map(n=16, order=4, remove="defocus")
    want2 = psfd.opd_map(n=7, order=3, remove=[(1, 1), (3, -1)], ref=(0.0, 1e-6), pupil=(0.0, 0.0, 0.05))
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
            got = sol.psf_opd_map(0, pos, ori, n=16, order=4, remove="defocus")
            assert sol.readout_ms > 0
            for a, b in zip(got, want):
                assert np.array_equal(a, b, equal_nan=True) and same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)), record
            got2 = sol.psf_opd_map(0, pos, ori, n=7, order=3, remove=[(1, 1), (3, -1)], ref=(0.0, 1e-6), pupil=(0.0, 0.0, 0.05))
            for a, b in zip(got2, want2):
                assert np.array_equal(a, b, equal_nan=True), record
        finally:
            sol.handle = None  # the engine frees the result
            eng.free_result(res)
    eng.free_batch(dev)
    eng.close()
