"""PSF read-out: intensity(psf) PSFDetector.jl:190-237.

CPU part: the oracle restatement reproduces the reference's Airy-disc KAT (test/runtests.jl:2764-2802).
GPU part: bmo_psf_intensity against the oracle on the same hits.  Oracle and kernel evaluate the same double-precision expression sequence
up to the argument of sincos, so only libm rounding and the re-association of the sum at split boundaries can differ; the field is held to

    |F_gpu - F_oracle| <= (12 + 2 H) u S,    u = 2^-53,  S = sum_h proj_h        (derivation: tests/readout_ref.py)

and the intensity to that times 2 |F|max.  The older check (1e-10 of the peak field magnitude, BASELINE.json's north_star for FP64) is kept
beside it.  The oracle's own sum is held to a 40-digit reference by tests/test_readout_reference.py.
"""
import math

import numpy as np
import pytest

import bmo_amd as bmo
import readout_ref as rr

RTOL = 1e-10


def airy_setup(num_rays=1000):
    # runtests.jl:2764-2784: almost thin plano-convex lens, plane wave, detector at the paraxial focus + 0.13 mm
    l, R1, R2, d, n, lam, D = 1e-3, 100e-3, math.inf, 25.4e-3, 1.5, 1e-6, 15e-3
    cs = bmo.UniformDiscSource([0, -10e-3, 0], [0, 1, 0], D, lam, num_rays=num_rays, e1=[1, 0, 0])
    lens = bmo.SphericalLens(R1, R2, l, d, lambda lam_: n)
    psfd = bmo.PSFDetector(10e-3)
    bmo.translate3d(psfd, [0, 200e-3 + 0.13e-3, 0])
    return bmo.System([lens, psfd]), cs, psfd, lam, D


def test_linrange_matches_julia_lerpi():
    xs = bmo.linalg.linrange(-1.0, 2.0, 4)
    assert xs.tolist() == [-1.0, (1 - 1 / 3) * -1.0 + (1 / 3) * 2.0, (1 - 2 / 3) * -1.0 + (2 / 3) * 2.0, 2.0]
    assert bmo.linalg.linrange(3.0, 5.0, 1).tolist() == [3.0]


def test_airy_disc_kat_oracle(oracle):
    """runtests.jl:2786-2802: first zero of the numerical PSF through the peak == 1.22 lambda f / D within 1 %."""
    system, cs, psfd, lam, D = airy_setup()
    oracle.solve_system(system, cs)
    assert len(psfd.data) == 1000  # runtests.jl:2806
    xs, zs, I = psfd.intensity(n=500, crop_factor=5, center="bbox",
                               _intensity_fn=lambda *a: oracle.psf_intensity(*a)[0])
    ix, jx = np.unravel_index(np.argmax(I), I.shape)
    num_min = xs[np.argmin(I[:, jx])]
    airy_min = 1.22 * lam * 200e-3 / D
    assert abs(abs(num_min) - airy_min) <= 1e-2 * airy_min
    psfd.empty()
    assert len(psfd.data) == 0


def test_psf_data_fields(oracle):
    """PSFData (PSFDetector.jl:77-89): hit on the detector plane, k = 2 pi / lambda, proj = |dir . n|, opl = sum n*l."""
    system, cs, psfd, lam, D = airy_setup(num_rays=64)
    oracle.solve_system(system, cs)
    d = psfd.data
    assert np.allclose(d[:, 1], 200e-3 + 0.13e-3, atol=1e-12)
    assert np.allclose(d[:, 8], 2 * math.pi / lam, rtol=0, atol=0)
    assert np.allclose(d[:, 7], np.abs(d[:, 4]), rtol=1e-15)  # detector normal is -y
    assert np.all(d[:, 6] > 0.21)  # > geometric path: 1 mm of glass at n = 1.5


def _assert_readout_matches_oracle(oracle, rows, pos, e1, e2, xs, zs, gpu):
    """(I_gpu, F_gpu) against the oracle on the same rows: the derived bound, and the older peak-relative one."""
    I_gpu, F_gpu = gpu
    I_ref, F_ref = oracle.psf_intensity(rows, pos, e1, e2, xs, zs)
    peak = np.abs(F_ref).max()
    S = float(rows[:, 7].sum())
    bound = rr.psf_engine_bound(rows)
    fmax = max(peak, np.abs(F_gpu).max())
    ef, ei = np.abs(F_gpu - F_ref).max(), np.abs(I_gpu - I_ref).max()
    print("H = %d, n = %d: |F_gpu - F_oracle| = %.3g S (bound %.3g S, peak %.3g S); |I_gpu - I_oracle| = %.3g (bound %.3g)"
          % (len(rows), len(xs), ef / S, bound / S, peak / S, ei, bound * 2 * fmax))
    assert peak > 0
    assert ef <= bound, (ef / S, bound / S)
    assert ei <= bound * 2 * fmax, (ei, bound * 2 * fmax)
    assert ef <= RTOL * peak
    assert ei <= 2 * RTOL * peak * peak
    assert np.array_equal(I_gpu, F_gpu.real ** 2 + F_gpu.imag ** 2)


def _airy_gpu_against_oracle(oracle, num_rays, n):
    system, cs, psfd, lam, D = airy_setup(num_rays=num_rays)
    bmo.solve_system(system, cs)  # the engine fills psfd.data
    assert len(psfd.data) == num_rays
    xs, zs = psfd.sample_axes(n=n, crop_factor=5, center="bbox") if num_rays > 1 else (bmo.linalg.linrange(-1e-5, 1e-5, n),) * 2
    o = psfd.orientation()
    I_gpu, F_gpu, ms = bmo.abi.psf_intensity(psfd.data, psfd.position(), o[:, 0], o[:, 2], xs, zs, want_field=True)
    _assert_readout_matches_oracle(oracle, psfd.data, psfd.position(), o[:, 0], o[:, 2], xs, zs, (I_gpu, F_gpu))


@pytest.mark.gpu
@pytest.mark.parametrize("num_rays,n", [(1000, 500), (300, 33), (1, 7)])
def test_gpu_psf_intensity_matches_oracle(oracle, num_rays, n):
    assert max(len(t) for t in rr.psf_tiles(num_rays, n * n)) == 1  # these shapes never reuse the LDS tile: the next test does
    _airy_gpu_against_oracle(oracle, num_rays, n)


@pytest.mark.gpu
@pytest.mark.parametrize("num_rays,n,what", [(5000, 500, "multi_tile"), (700, 13, "ragged_grid"), (1 << 18, 7, "many_splits")])
def test_gpu_psf_intensity_tile_loop_and_split_shapes_match_oracle(oracle, num_rays, n, what):
    tiles = rr.psf_tiles(num_rays, n * n)
    if what == "multi_tile":  # the tile loop of psf_sum_range makes a third trip, in several splits, and ends on a partial tile
        assert len(tiles) >= 2 and min(len(t) for t in tiles) >= 3 and tiles[-1][-1] < rr.PSF_TILE
    elif what == "ragged_grid":  # the last lanes of the only point block are past the grid; several splits, a partial last tile
        assert (n * n) % 256 != 0 and n < 16 and len(tiles) >= 2 and tiles[-1][-1] < rr.PSF_TILE
    else:  # one point block, a thousand split rows for the reduce kernel
        assert n * n <= 256 and len(tiles) >= 1000
    _airy_gpu_against_oracle(oracle, num_rays, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 40])
@pytest.mark.parametrize("null_hits", [False, True])
def test_gpu_psf_intensity_without_hits_is_exactly_zero(n, null_hits):
    """n_hits = 0 through the raw ABI, the output buffers filled with NaN beforehand: the kernels themselves must write the +0."""
    import ctypes as C

    lib = bmo.abi.load_engine()
    dp = C.POINTER(C.c_double)
    xs, zs = bmo.linalg.linrange(-1e-5, 1e-5, n), bmo.linalg.linrange(-2e-5, 1e-5, n)
    o, e1, e2 = np.array([0, 0.2, 0.0]), np.array([-1.0, 0, 0]), np.array([0, 0, 1.0])
    I, F = np.full(n * n, np.nan), np.full(2 * n * n, np.nan)
    rows = np.zeros((1, 9))  # a valid pointer that must not be read
    ms = C.c_double()
    rc = lib.bmo_psf_intensity(None if null_hits else rows.ctypes.data_as(C.c_void_p), 0, 0, o.ctypes.data_as(dp), e1.ctypes.data_as(dp),
                               e2.ctypes.data_as(dp), xs.ctypes.data_as(dp), zs.ctypes.data_as(dp), n, 0, I.ctypes.data_as(dp), F.ctypes.data_as(dp), C.byref(ms))
    assert rc == 0, lib.bmo_last_error()
    assert not np.isnan(I).any() and not np.isnan(F).any()  # every entry was written
    assert not I.any() and not F.any()
    assert not np.signbit(I).any() and not np.signbit(F).any()  # +0, not -0
    # and the wrapper, which shapes the result
    I2, F2, _ = bmo.abi.psf_intensity(np.zeros((0, 9)), o, e1, e2, xs, zs, want_field=True)
    assert I2.shape == (n, n) and F2.shape == (n, n) and not I2.any() and not F2.any()


@pytest.mark.gpu
@pytest.mark.parametrize("num_rays,n", [(3000, 500), (700, 13)])
def test_gpu_psf_intensity_on_a_tilted_decentred_detector(oracle, num_rays, n):
    """No zero in e1, e2 or the hit directions (the Airy scene has e1 = x, e2 = z): host rows and the rows still resident in HBM."""
    if num_rays == 3000:  # three tiles per split here too
        assert min(len(t) for t in rr.psf_tiles(num_rays, n * n)) >= 3
    system, psfd, bundle = rr.tilted_psf_case(num_rays)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    try:
        dev = eng.upload(bundle)
        res = eng.trace_device(dev, 100)
        ptr, cnt = eng.result_device_hits(res, 0)
        assert cnt == num_rays
        rows = eng.result_view(res).detector_hits(0).copy()
        pos, o = np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)
        e1, e2 = o[:, 0].copy(), o[:, 2].copy()
        assert np.all(np.abs(e1) > 1e-3) and np.all(np.abs(e2) > 1e-3), (e1, e2)
        assert (rows[:, 3:6] != 0).all()
        xs, zs = bmo.components.psf_sample_axes(rows, pos, o, n=n, crop_factor=5, center="bbox")
        I_h, F_h, _ = bmo.abi.psf_intensity(rows, pos, e1, e2, xs, zs, want_field=True)
        I_d, F_d, _ = bmo.abi.psf_intensity(None, pos, e1, e2, xs, zs, hits_device_ptr=ptr, n_hits=cnt, want_field=True)
        assert np.array_equal(I_h, I_d) and np.array_equal(F_h, F_d)
        _assert_readout_matches_oracle(oracle, rows, pos, e1, e2, xs, zs, (I_d, F_d))
        # the rows themselves are the oracle's, bit for bit
        ref = oracle.trace(scene, bundle, 100)
        assert np.array_equal(ref.detector_hits(0), rows)
        eng.free_result(res)
        eng.free_batch(dev)
    finally:
        eng.close()


@pytest.mark.gpu
def test_gpu_psf_intensity_device_resident_hits_and_airy_kat(oracle):
    """Same KAT as the CPU test, read out by the engine from the hit buffer that is still resident in HBM."""
    system, cs, psfd, lam, D = airy_setup()
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100)
    ptr, cnt = eng.result_device_hits(res, 0)
    assert cnt == 1000
    view = eng.result_view(res)
    psfd.data = view.detector_hits(0).copy()
    xs, zs = psfd.sample_axes(n=500, crop_factor=5, center="bbox")
    o = psfd.orientation()
    I, _, ms = bmo.abi.psf_intensity(None, psfd.position(), o[:, 0], o[:, 2], xs, zs, hits_device_ptr=ptr, n_hits=cnt)
    I_host, _, _ = bmo.abi.psf_intensity(psfd.data, psfd.position(), o[:, 0], o[:, 2], xs, zs)
    assert np.array_equal(I, I_host)
    ix, jx = np.unravel_index(np.argmax(I), I.shape)
    num_min = xs[np.argmin(I[:, jx])]
    airy_min = 1.22 * lam * 200e-3 / D
    assert abs(abs(num_min) - airy_min) <= 1e-2 * airy_min
    eng.free_result(res)
    eng.free_batch(dev)
    eng.close()


@pytest.mark.gpu
def test_gpu_psf_intensity_rejects_bad_arguments():
    with pytest.raises(RuntimeError):
        bmo.abi.psf_intensity(np.zeros((3, 9)), [0, 0, 0], [1, 0, 0], [0, 0, 1], [0.0, 1.0], [0.0, 1.0], device=99)
