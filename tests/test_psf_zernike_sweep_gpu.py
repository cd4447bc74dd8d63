"""Zernike read-out of sweeps on the GPU: SweepSolution.psf_zernike (bmo_psf_zernike_sweep) equals, configuration by configuration and bit
for bit, bmo_psf_zernike on that configuration's rows.  The scenes are those of test_psf_stats_sweep_gpu.py: K = 1, 3, 8, ragged counts, one
configuration that records nothing, a pose per configuration."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import zernike_ref as zr
from test_psf_readout import airy_setup
from test_psf_stats import same_bits
from test_psf_stats_sweep_gpu import PLACES, _pose, _sweep, mm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[1, 3, 8])
def swept(request):
    K = request.param
    sol, psfd = _sweep(K)
    rows = [sol.detector_hits(psfd, c).copy() for c in range(K)]
    yield K, sol, psfd, rows
    sol.close()


def test_every_configuration_equals_the_single_call(swept):
    K, sol, psfd, rows = swept
    counts = [len(r) for r in rows]
    print("K = %d, rows per configuration: %s" % (K, counts))
    if K > 1:
        assert 0 in counts and len(set(counts)) >= 3, counts
    for order, ref, pupil in ((4, None, None), (2, (1e-6, -2e-6), None), (6, None, (1e-3, 0.0, 0.06))):
        coef, info, gram = sol.psf_zernike(psfd, order=order, ref=ref, pupil=pupil, want_gram=True)
        J, E = abi.zernike_sizes(order)
        assert coef.shape == (K, J) and info.shape == (K, abi.ZERN_INFO_N) and gram.shape == (K, E) and sol.readout_ms > 0
        c2, i2 = sol.psf_zernike(psfd, order=order, ref=ref, pupil=pupil)
        assert same_bits(c2, coef) and same_bits(i2, info)
        for c in range(K):
            sc, si, sg, _ = abi.psf_zernike(rows[c], *_pose(sol, psfd, c), order=order, ref=ref, pupil=pupil, want_gram=True)
            assert same_bits(coef[c], sc) and same_bits(info[c], si) and same_bits(gram[c], sg), (order, c)
            if counts[c] == 0:
                assert info[c, zr.N] == 0 and info[c, zr.STATUS] == 1 and np.isnan(np.delete(info[c], [zr.N, zr.STATUS])).all()
                assert np.isnan(coef[c]).all() and np.isnan(gram[c]).all()
            else:
                assert info[c, zr.N] == counts[c]
                if pupil is None:  # the rows fill their own pupil
                    assert info[c, zr.STATUS] == 0 and np.isfinite(coef[c]).all(), (order, c)
    if K == 8:
        _check_defocus_through_focus(sol, psfd)
    # a reference point and a pupil per configuration
    if K > 1:
        ref = np.column_stack([1e-6 * np.arange(K), -1e-6 * np.ones(K)])
        pupil = np.column_stack([1e-3 * np.arange(K), np.zeros(K), 0.05 + 1e-3 * np.arange(K)])
        coef, info = sol.psf_zernike(psfd, order=3, ref=ref, pupil=pupil)
        for c in range(K):
            sc, si, _, _ = abi.psf_zernike(rows[c], *_pose(sol, psfd, c), order=3, ref=ref[c], pupil=pupil[c])
            assert same_bits(coef[c], sc) and same_bits(info[c], si), c


def test_detector_only_result_reads_the_same(swept):
    K, sol, psfd, rows = swept
    sol0, psfd0 = _sweep(K, record_segments=False)
    try:
        a, b = sol0.psf_zernike(psfd0, order=4, want_gram=True), sol.psf_zernike(psfd, order=4, want_gram=True)
        assert all(same_bits(x, y) for x, y in zip(a, b))
    finally:
        sol0.close()


def _check_defocus_through_focus(sol, psfd):
    """The on-axis places of K = 8 from y = 199 mm on scan the focus: the reference point (the centroid) passes the focus along the axis, and
    the defocus coefficient c(Z_2^0) of the path to it is strictly monotonic in y."""
    coef, info = sol.psf_zernike(psfd, order=4)
    on_axis = sorted((y, c) for c, (x, y) in enumerate(PLACES[8]) if x == 0.0 and y >= 199 * mm)
    assert len(on_axis) >= 4
    d = [coef[c, zr.term_index(2, 0)] for y, c in on_axis]
    print("defocus through focus: " + "  ".join("y = %.2f mm: %.4g m" % (y / mm, v) for (y, c), v in zip(on_axis, d)))
    steps = np.diff(d)
    assert np.all(steps > 0) or np.all(steps < 0), d
    assert min(d) < 0 < max(d)


def _raw(handle, slot, K, order=2, origin=True, coef=True, info=True, pupil=None):
    lib = abi.load_engine()
    dp = C.POINTER(C.c_double)
    K1 = max(K, 1)
    o, e1, e2 = np.zeros((K1, 3)), np.tile([1.0, 0, 0], (K1, 1)), np.tile([0, 0, 1.0], (K1, 1))
    cf, nf = np.zeros((K1, 28)), np.zeros((K1, abi.ZERN_INFO_N))
    q = None if pupil is None else np.ascontiguousarray(np.tile(np.asarray(pupil, dtype=np.float64), (K1, 1)))
    return lib.bmo_psf_zernike_sweep(handle, slot, K, o.ctypes.data_as(dp) if origin else None, e1.ctypes.data_as(dp), e2.ctypes.data_as(dp), None,
                                     None if q is None else q.ctypes.data_as(dp), order, cf.ctypes.data_as(dp) if coef else None,
                                     nf.ctypes.data_as(dp) if info else None, None, None)


def test_wrong_slot_order_pupil_and_configuration_count_are_refused():
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
        assert _raw(sol._handle, ps, 3) == 0
        assert _raw(sol._handle, ss, 3) == -1  # a Spotdetector's slot
        assert "PSFDetector" in abi.load_engine().bmo_last_error().decode()
        for bad_k in (1, 2, 4, 0):
            assert _raw(sol._handle, ps, bad_k) == -1, bad_k
        assert _raw(sol._handle, 7, 3) == -1 and _raw(sol._handle, -1, 3) == -1
        assert _raw(sol._handle, ps, 3, origin=False) == -1 and _raw(sol._handle, ps, 3, coef=False) == -1 and _raw(sol._handle, ps, 3, info=False) == -1
        assert _raw(sol._handle, ps, 3, order=7) == -1 and _raw(sol._handle, ps, 3, order=-1) == -1
        assert _raw(sol._handle, ps, 3, pupil=(0.0, 0.0, 0.0)) == -1 and _raw(sol._handle, ps, 3, pupil=(np.nan, 0.0, 0.05)) == -1
        assert _raw(sol._handle, ps, 3, pupil=(0.0, 0.0, 0.05)) == 0
        with pytest.raises(RuntimeError, match="bmo_psf_zernike_sweep"):
            sol.psf_zernike(spot)
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
