"""PSF read-out of sweeps, the parts that need no GPU: the sampling window as a function of (rows, pose) and the argument checks of
bmo_psf_intensity_sweep."""
import ctypes as C
import itertools
import math

import numpy as np

import bmo_amd as bmo
from bmo_amd import abi


def _window_as_written(rows, position, orientation, n, crop_factor=1.0, center="centroid", x_min=math.inf, x_max=math.inf, z_min=math.inf,
                       z_max=math.inf, x0_shift=0.0, z0_shift=0.0):
    """PSFDetector.calc_local_pos / calc_local_lims / sample_axes (PSFDetector.jl:91-144, :205-217) as they read before the window became a
    module-level function."""
    loc = rows[:, 0:3] - position[None, :]
    hits = np.stack([loc @ orientation[:, 0], loc @ orientation[:, 2]], axis=1)
    xs, zs = hits[:, 0], hits[:, 1]
    if center == "centroid":
        w = rows[:, 7]
        w_sum = w.sum()
        x0, z0 = (w * xs).sum() / w_sum, (w * zs).sum() / w_sum
    else:
        x0, z0 = (xs.min() + xs.max()) / 2, (zs.min() + zs.max()) / 2
    hwx, hwy = np.abs(xs - x0).max() * crop_factor, np.abs(zs - z0).max() * crop_factor
    lx, hx, lz, hz = x0 - hwx, x0 + hwx, z0 - hwy, z0 + hwy
    if x_min != math.inf and x_max != math.inf:
        lx, hx = x_min, x_max
    if z_min != math.inf and z_max != math.inf:
        lz, hz = z_min, z_max
    return bmo.linalg.linrange(lx, hx, n) + x0_shift, bmo.linalg.linrange(lz, hz, n) + z0_shift


def _random_rows(rng, H, position):
    rows = np.zeros((H, 9))
    rows[:, 0:3] = position[None, :] + 1e-3 * rng.standard_normal((H, 3))
    d = rng.standard_normal((H, 3))
    rows[:, 3:6] = d / np.linalg.norm(d, axis=1)[:, None]
    rows[:, 6] = 0.2 + 1e-6 * rng.random(H)
    rows[:, 7] = rng.random(H) + 0.1
    rows[:, 8] = 2 * math.pi / 1e-6
    return rows


def test_window_function_equals_sample_axes_bit_for_bit():
    rng = np.random.Generator(np.random.PCG64(11))
    kws = []
    for center, crop, lims, shifts in itertools.product(("centroid", "bbox"), (1, 1.0, 2.5, 0.3),
                                                        (None, "x", "z", "xz", "x_half"), ((0, 0), (0.0, 0.0), (1e-5, -3e-6))):
        kw = dict(center=center, crop_factor=crop, x0_shift=shifts[0], z0_shift=shifts[1])
        if lims in ("x", "xz"):
            kw.update(x_min=-2e-4, x_max=3e-4)
        if lims in ("z", "xz"):
            kw.update(z_min=-1e-4, z_max=5e-4)
        if lims == "x_half":  # only one limit of an axis given: the reference ignores it
            kw.update(x_min=-2e-4)
        kws.append(kw)
    for trial in range(12):
        psfd = bmo.PSFDetector(10e-3)
        bmo.translate3d(psfd, list(rng.uniform(-0.1, 0.1, 3)))
        bmo.xrotate3d(psfd, float(rng.uniform(-math.pi, math.pi)))
        bmo.zrotate3d(psfd, float(rng.uniform(-math.pi, math.pi)))
        psfd.data = _random_rows(rng, int(rng.integers(1, 300)), np.asarray(psfd.position()))
        # the pose as a sweep keeps it: copies of the numbers
        pos, ori = np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)
        n = int(rng.integers(1, 70))
        for kw in kws:
            want = _window_as_written(psfd.data, pos, ori, n, **kw)
            got_fn = bmo.components.psf_sample_axes(psfd.data, pos, ori, n=n, **kw)
            got_method = psfd.sample_axes(n=n, **kw)
            for w, f, m in zip(want, got_fn, got_method):
                assert np.array_equal(w, f) and np.array_equal(w, m), (trial, kw)
                assert np.array_equal(np.signbit(w), np.signbit(f))
        lims = psfd.calc_local_lims(crop_factor=1.7, center="bbox")
        assert lims == bmo.components.psf_local_lims(psfd.data, pos, ori, crop_factor=1.7, center="bbox")
        assert np.array_equal(psfd.calc_local_pos(), bmo.components.psf_local_pos(psfd.data, pos, ori))


def test_psf_intensity_sweep_refuses_bad_arguments_without_a_device():
    lib = abi.load_engine()
    dp = C.POINTER(C.c_double)
    v3 = np.zeros(3)
    ax = np.linspace(-1e-4, 1e-4, 8)
    out, fld = np.zeros(64), np.zeros(128)
    ms = C.c_double()
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    # a null result
    assert lib.bmo_psf_intensity_sweep(None, 0, 1, p(v3), p(v3), p(v3), p(ax), p(ax), 8, p(out), p(fld), C.byref(ms)) == -1
    assert "bmo_psf_intensity_sweep" in lib.bmo_last_error().decode()
    # n <= 0
    for n in (0, -3):
        assert lib.bmo_psf_intensity_sweep(None, 0, 1, p(v3), p(v3), p(v3), p(ax), p(ax), n, p(out), None, None) == -1
    # null arrays
    assert lib.bmo_psf_intensity_sweep(None, 0, 1, None, p(v3), p(v3), p(ax), p(ax), 8, p(out), None, None) == -1
    assert lib.bmo_psf_intensity_sweep(None, 0, 1, p(v3), p(v3), p(v3), p(ax), p(ax), 8, None, None, None) == -1
