"""OPD map read-out of sweeps on the GPU: SweepSolution.psf_opd_map (bmo_psf_opd_map_sweep) equals, configuration by configuration and bit
for bit in all five outputs, bmo_psf_opd_map on that configuration's rows; the scenes are those of test_psf_stats_sweep_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import opd_ref as od
from test_psf_readout import airy_setup
from test_psf_stats import same_bits
from test_psf_stats_sweep_gpu import _pose, _sweep

pytestmark = pytest.mark.gpu
mm = 1e-3
N_BINS = 7


@pytest.fixture(scope="module", params=[1, 3, 8])
def swept(request):
    K = request.param
    sol, psfd = _sweep(K)
    rows = [sol.detector_hits(psfd, c).copy() for c in range(K)]
    yield K, sol, psfd, rows
    sol.close()


def _same(got, want, what):
    """the five outputs of one configuration: opd, weight, count, info, raw"""
    for a, b in zip(got[:5], want[:5]):
        assert a.shape == b.shape and a.dtype == b.dtype, what
        assert np.array_equal(a, b, equal_nan=True) and same_bits(a.astype(np.float64), b.astype(np.float64)), what


def test_every_configuration_equals_the_single_call(swept):
    K, sol, psfd, rows = swept
    counts = [len(r) for r in rows]
    print("K = %d, rows per configuration: %s" % (K, counts))
    if K > 1:
        assert 0 in counts and len(set(counts)) >= 3, counts  # one records nothing, the counts are ragged
    slot = sol._slot(psfd)
    pos = np.ascontiguousarray([sol._poses[c][slot][0] for c in range(K)], dtype=np.float64)
    ori = np.ascontiguousarray([sol._poses[c][slot][1] for c in range(K)], dtype=np.float64)
    rng = np.random.default_rng(4)
    refs = np.column_stack([1e-6 * rng.uniform(-1, 1, K), 1e-6 * rng.uniform(-1, 1, K)])
    pupils = np.column_stack([1e-3 * rng.uniform(-1, 1, K), 1e-3 * rng.uniform(-1, 1, K), 0.04 + 0.01 * rng.uniform(0, 1, K)])
    coefs = 1e-8 * rng.uniform(-1, 1, (K, 6))
    for n in (N_BINS, 65):  # LDS and global memory
        for ref, pupil, order, coef in ((None, None, 0, None), (refs[0], pupils[0], 2, coefs[0]), (refs, pupils, 2, coefs), (None, pupils, 2, coefs[0])):
            got = abi.psf_opd_map_sweep(sol._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], n=n, order=order, coef=coef, ref=ref, pupil=pupil, want_raw=True)
            assert got[0].shape == (K, n, n) and got[3].shape == (K, od.INFO_N) and got[4].shape == (K, n, n, 2) and got[5] > 0
            for c in range(K):
                pick = lambda v: None if v is None else (v if np.ndim(v) == 1 else v[c])  # noqa: E731
                want = abi.psf_opd_map(rows[c], *_pose(sol, psfd, c), n=n, order=order, coef=pick(coef), ref=pick(ref), pupil=pick(pupil), want_raw=True)
                _same([g[c] for g in got[:5]], want, (n, c, order))
                info = got[3][c]
                if counts[c] == 0:
                    assert info[od.N] == 0 and info[od.STATUS] == 1 and np.isnan(got[0][c]).all() and not got[2][c].any()
                else:
                    assert info[od.N] == counts[c] and int(got[2][c].sum()) + info[od.N_OUTSIDE] == counts[c]
    # the Python layer: one fit and one map for all configurations
    opd, weight, count, info, removed = sol.psf_opd_map(psfd, n=N_BINS, order=2, remove="tilt")
    assert opd.shape == (K, N_BINS, N_BINS) and removed.shape == (K, 6) and sol.readout_ms > 0
    for c in range(K):
        if counts[c] >= 6:
            w = bmo.components.psf_opd_map(lambda o_, r, q: abi.psf_zernike(rows[c], *_pose(sol, psfd, c), order=o_, ref=r, pupil=q)[:2],
                                           lambda o_, cf, r, q: abi.psf_opd_map(rows[c], *_pose(sol, psfd, c), n=N_BINS, order=o_, coef=cf, ref=r, pupil=q)[:4],
                                           n=N_BINS, order=2, remove="tilt")
            assert same_bits(opd[c], w[0]) and np.array_equal(count[c], w[2]) and same_bits(info[c], w[3]) and same_bits(removed[c], w[4])
        elif counts[c] == 0:
            assert info[c, od.STATUS] == 1 and np.isnan(opd[c]).all()
    given = sol.psf_opd_map(psfd, n=N_BINS, order=2, coef=coefs, ref=refs, pupil=pupils)
    direct = abi.psf_opd_map_sweep(sol._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], n=N_BINS, order=2, coef=coefs, ref=refs, pupil=pupils)
    assert same_bits(given[0], direct[0]) and same_bits(given[3], direct[3]) and same_bits(given[4], coefs)


def test_detector_only_result_reads_the_same(swept):
    K, sol, psfd, rows = swept
    sol0, psfd0 = _sweep(K, record_segments=False)
    try:
        a, b = sol0.psf_opd_map(psfd0, n=N_BINS, order=2, remove="defocus"), sol.psf_opd_map(psfd, n=N_BINS, order=2, remove="defocus")
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True) and same_bits(x.astype(np.float64), y.astype(np.float64))
    finally:
        sol0.close()


def _raw(handle, slot, K, n=4, origin=True, opd=True, order=0, coef=None):
    """the return code of the sweep entry, and that a refused call left the caller's buffers alone"""
    lib = abi.load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    K1, nb = max(K, 1), min(max(n, 1), 64) ** 2
    o, e1, e2 = np.zeros((K1, 3)), np.tile([1.0, 0, 0], (K1, 1)), np.tile([0, 0, 1.0], (K1, 1))
    a_opd, a_w, a_cnt, a_raw, a_info = np.full((K1, nb), 7.0), np.full((K1, nb), 7.0), np.full((K1, nb), 7, dtype=np.int64), np.full((K1, nb, 2), 7, dtype=np.int64), \
        np.full((K1, od.INFO_N), 7.0)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    rc = lib.bmo_psf_opd_map_sweep(handle, slot, K, o.ctypes.data_as(dp) if origin else None, e1.ctypes.data_as(dp), e2.ctypes.data_as(dp), None, None, order,
                                   None if cf is None else cf.ctypes.data_as(dp), n, a_opd.ctypes.data_as(dp) if opd else None, a_w.ctypes.data_as(dp),
                                   a_cnt.ctypes.data_as(ip), a_raw.ctypes.data_as(ip), a_info.ctypes.data_as(dp), None)
    if rc != 0:
        assert (a_opd == 7).all() and (a_w == 7).all() and (a_cnt == 7).all() and (a_raw == 7).all() and (a_info == 7).all()
    else:
        assert (a_info[:, od.STATUS] != 7).all()
    return rc


def test_refusals():
    system, cs, psfd, lam, D = airy_setup(num_rays=64)
    spot = bmo.Spotdetector(5 * mm)
    bmo.translate3d(spot, [50 * mm, 0, 0])
    system = bmo.System(list(system.objects()) + [spot])
    p0 = np.array(psfd.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(psfd, list(p0 + np.array([0, 0.1 * mm * c, 0])))

    sol = bmo.solve_sweep(system, cs, 3, configure)
    try:
        ps, ss = sol._slot(psfd), sol._slot(spot)
        err = lambda: abi.load_engine().bmo_last_error().decode()  # noqa: E731
        assert _raw(sol._handle, ps, 3) == 0
        assert _raw(sol._handle, ss, 3) == -1 and "PSFDetector" in err()  # a Spotdetector's slot
        for bad_k in (1, 2, 4, 0):
            assert _raw(sol._handle, ps, bad_k) == -1, bad_k
        assert _raw(sol._handle, 7, 3) == -1 and _raw(sol._handle, -1, 3) == -1
        assert _raw(sol._handle, ps, 3, origin=False) == -1 and _raw(sol._handle, ps, 3, opd=False) == -1
        assert _raw(sol._handle, ps, 3, n=0) == -1 and "bins per axis" in err()
        assert _raw(sol._handle, ps, 3, n=abi.OPD_MAX_N + 1) == -1 and _raw(sol._handle, ps, 3, n=-1) == -1
        assert _raw(sol._handle, ps, 3, order=2) == -1 and "NULL" in err()  # no coefficients at order 2
        assert _raw(sol._handle, ps, 3, order=7, coef=np.zeros((3, 36))) == -1
        assert _raw(sol._handle, ps, 3, order=1, coef=[[0, 0, 0], [0, np.nan, 0], [0, 0, 0]]) == -1 and "finite" in err()
        assert _raw(sol._handle, ps, 3, order=1, coef=np.zeros((3, 3))) == 0
        with pytest.raises(RuntimeError, match="bmo_psf_opd_map_sweep"):
            sol.psf_opd_map(spot, remove="none")
        with pytest.raises(RuntimeError, match="bins per axis"):
            sol.psf_opd_map(psfd, n=0)
    finally:
        sol.close()


def test_a_gaussian_result_is_unsupported():
    import scenes

    system, _ = scenes.c2_scene()
    b = scenes.c3_bundle(64)
    sc = bmo.CompiledScene(system, b.lambdas)
    res, sol = bmo.system._engine_solve(sc, b, 100, None)
    try:
        assert _raw(sol.handle, 0, 1) == -4
        assert "GaussianBeamlet" in abi.load_engine().bmo_last_error().decode()
    finally:
        sol.free()
