"""PSF read-out of sweeps on the GPU: SweepSolution.psf_intensity / bmo_psf_intensity_sweep equals, configuration by configuration and bit
for bit, bmo_psf_intensity on that configuration's rows (and a fresh solve of its snapshot followed by PSFDetector.intensity)."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
from test_psf_readout import RTOL, airy_setup

pytestmark = pytest.mark.gpu
mm = 1e-3


def _airy_sweep(num_rays, dys):
    """The Airy KAT scene with its PSFDetector at the nominal position + dys[c] along the axis in configuration c."""
    system, cs, psfd, lam, D = airy_setup(num_rays=num_rays)
    p0 = np.array(psfd.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(psfd, list(p0 + np.array([0, dys[c], 0])))

    return bmo.solve_sweep(system, cs, len(dys), configure), psfd, p0


def _pose(sol, det, c):
    pos, ori = sol._poses[c][sol._slot(det)]
    return pos, ori[:, 0], ori[:, 2]


def _single(sol, det, c, xs, zs):
    pos, e1, e2 = _pose(sol, det, c)
    I, F, _ = abi.psf_intensity(sol.detector_hits(det, c), pos, e1, e2, xs, zs, want_field=True)
    return I, F


def _raw(sol_handle, slot, K, n):
    """bmo_psf_intensity_sweep's return code on a K x n request."""
    lib = abi.load_engine()
    dp = C.POINTER(C.c_double)
    K1 = max(K, 1)
    o, e1, e2 = np.zeros((K1, 3)), np.tile([1.0, 0, 0], (K1, 1)), np.tile([0, 0, 1.0], (K1, 1))
    ax = np.tile(np.linspace(-1e-4, 1e-4, n), (K1, 1))
    out = np.zeros(K1 * n * n)
    return lib.bmo_psf_intensity_sweep(sol_handle, slot, K, o.ctypes.data_as(dp), e1.ctypes.data_as(dp), e2.ctypes.data_as(dp),
                                       ax.ctypes.data_as(dp), ax.ctypes.data_as(dp), n, out.ctypes.data_as(dp), None, None)


def test_through_focus_scan_equals_single_calls_fresh_solves_and_the_oracle(oracle):
    K, n = 9, 64
    dys = bmo.linalg.linrange(-1 * mm, 1 * mm, K)
    sol, psfd, p0 = _airy_sweep(1000, dys)
    try:
        xs, zs, I, F = sol.psf_intensity(psfd, n=n, want_field=True)
        assert xs.shape == (K, n) and zs.shape == (K, n) and I.shape == (K, n, n) and F.shape == (K, n, n)
        for c in range(K):
            rows = sol.detector_hits(psfd, c)
            assert len(rows) == 1000
            pos, e1, e2 = _pose(sol, psfd, c)
            ax, az = bmo.components.psf_sample_axes(rows, pos, sol._poses[c][sol._slot(psfd)][1], n=n)
            assert np.array_equal(xs[c], ax) and np.array_equal(zs[c], az)
            I1, F1 = _single(sol, psfd, c, xs[c], zs[c])
            assert np.array_equal(I[c], I1), c
            assert np.array_equal(F[c], F1), c
            # a fresh solve of snapshot c, read the way a user reads one PSF
            system2, cs2, psfd2, _, _ = airy_setup(num_rays=1000)
            bmo.translate_to3d(psfd2, list(p0 + np.array([0, dys[c], 0])))
            bmo.solve_system(system2, cs2)
            fx, fz, fI = psfd2.intensity(n=n)
            assert np.array_equal(fx, xs[c]) and np.array_equal(fz, zs[c]) and np.array_equal(fI, I[c]), c
            I_ref, F_ref = oracle.psf_intensity(rows, pos, e1, e2, xs[c], zs[c])
            peak = np.abs(F_ref).max()
            assert np.abs(F[c] - F_ref).max() <= RTOL * peak, c
            assert np.abs(I[c] - I_ref).max() <= 2 * RTOL * peak * peak, c
        # the focus is inside the scan: the peak intensity is largest away from the ends
        peaks = I.max(axis=(1, 2))
        assert peaks.argmax() not in (0, K - 1)
        # without want_field: the same intensities
        xs2, zs2, I2 = sol.psf_intensity(psfd, n=n)
        assert np.array_equal(I2, I) and np.array_equal(xs2, xs)
    finally:
        sol.close()


def test_unequal_and_empty_configurations():
    """A 4 mm detector in a 15 mm collimated beam, moved sideways: the row counts differ and configuration 3 records no hit."""
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 15 * mm, 1e-6, num_rays=2000, e1=[1, 0, 0])
    psfd = bmo.PSFDetector(4 * mm)
    bmo.translate3d(psfd, [0, 50 * mm, 0])
    system = bmo.System([psfd])
    xoff = [0.0, 3 * mm, 5.5 * mm, 30 * mm]

    def configure(c):
        bmo.translate_to3d(psfd, [xoff[c], 50 * mm, 0])

    sol = bmo.solve_sweep(system, cs, len(xoff), configure)
    try:
        counts = [len(sol.detector_hits(psfd, c)) for c in range(len(xoff))]
        assert counts[3] == 0 and len(set(counts[:3])) == 3 and min(counts[:3]) > 0, counts
        with pytest.raises(ValueError, match="configuration 3"):
            sol.psf_intensity(psfd, n=32)
        ax = bmo.linalg.linrange(-2 * mm, 2 * mm, 32)
        az = bmo.linalg.linrange(-1.5 * mm, 2.5 * mm, 32)
        xs, zs, I, F = sol.psf_intensity(psfd, n=32, axes=(ax, az), want_field=True)
        assert np.array_equal(xs, np.tile(ax, (4, 1))) and np.array_equal(zs, np.tile(az, (4, 1)))
        for c in range(3):
            I1, F1 = _single(sol, psfd, c, ax, az)
            assert np.array_equal(I[c], I1) and np.array_equal(F[c], F1), c
        # the empty configuration reads like a single call with n_hits = 0
        I0, F0 = _single(sol, psfd, 3, ax, az)
        assert np.array_equal(I[3], I0) and np.array_equal(F[3], F0)
        assert not I[3].any() and not F[3].any()
        assert not np.signbit(I[3]).any()
    finally:
        sol.close()


def test_many_splits_per_configuration():
    """2^16 rows per configuration on a 100 x 100 grid: bmo_psf_intensity splits each into many workgroup rows."""
    K, n = 4, 100
    sol, psfd, _ = _airy_sweep(1 << 16, bmo.linalg.linrange(-0.3 * mm, 0.3 * mm, K))
    try:
        xs, zs, I, F = sol.psf_intensity(psfd, n=n, crop_factor=2, center="bbox", want_field=True)
        for c in range(K):
            assert len(sol.detector_hits(psfd, c)) == 1 << 16
            I1, F1 = _single(sol, psfd, c, xs[c], zs[c])
            assert np.array_equal(I[c], I1) and np.array_equal(F[c], F1), c
    finally:
        sol.close()


def test_more_configurations_than_one_launch_holds():
    """150 configurations x 4 096 rows on a 256 x 256 grid: 16 splits and 16 MiB of partial sums per configuration, so the 1 GiB cap of
    one launch splits the read-out into three."""
    K, n = 150, 256
    sol, psfd, _ = _airy_sweep(4096, bmo.linalg.linrange(-0.5 * mm, 0.5 * mm, K))
    try:
        xs, zs, I = sol.psf_intensity(psfd, n=n, x0_shift=1e-6)
        assert I.shape == (K, n, n)
        for c in (0, 1, 40, 63, 64, 65, 100, 127, 128, 129, 148, 149):
            assert len(sol.detector_hits(psfd, c)) == 4096
            I1, _ = _single(sol, psfd, c, xs[c], zs[c])
            assert np.array_equal(I[c], I1), c
    finally:
        sol.close()


def test_wrong_slot_and_configuration_count_are_refused():
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
        assert _raw(sol._handle, ps, 3, 8) == 0
        assert _raw(sol._handle, ss, 3, 8) == -1  # a Spotdetector's slot
        assert "PSFDetector" in abi.load_engine().bmo_last_error().decode()
        for bad_k in (1, 2, 4, 0):
            assert _raw(sol._handle, ps, bad_k, 8) == -1, bad_k
        assert _raw(sol._handle, 7, 3, 8) == -1
        assert _raw(sol._handle, -1, 3, 8) == -1
        assert _raw(sol._handle, ps, 3, 0) == -1
        with pytest.raises(RuntimeError, match="bmo_psf_intensity_sweep"):
            sol.psf_intensity(spot, n=8, axes=(np.zeros(8), np.zeros(8)))
    finally:
        sol.close()


def test_ordinary_result_with_one_configuration():
    system, cs, psfd, lam, D = airy_setup(num_rays=1000)
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100)
    try:
        rows = eng.result_view(res).detector_hits(0)
        assert len(rows) == 1000
        pos, ori = np.array(psfd.position()), np.array(psfd.orientation())
        xs, zs = bmo.components.psf_sample_axes(rows, pos, ori, n=64, crop_factor=5, center="bbox")
        I, F, ms = abi.psf_intensity_sweep(res, 0, 1, pos, ori[:, 0], ori[:, 2], xs, zs, want_field=True)
        I1, F1, _ = abi.psf_intensity(rows, pos, ori[:, 0], ori[:, 2], xs, zs, want_field=True)
        assert np.array_equal(I[0], I1) and np.array_equal(F[0], F1)
        assert ms > 0
        assert _raw(res, 0, 2, 8) == -1  # an ordinary result has one configuration
    finally:
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()
