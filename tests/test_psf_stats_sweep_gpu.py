"""Wavefront read-out of sweeps on the GPU: SweepSolution.psf_stats (bmo_psf_stats_sweep) equals, configuration by configuration and bit
for bit, bmo_psf_stats on that configuration's rows; psf_intensity(window="device") reads every configuration on the axes those statistics
give, without a host copy of the rows."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import psf_stats_ref as pr
import readout_ref as rr
from test_psf_readout import airy_setup
from test_psf_stats import same_bits

pytestmark = pytest.mark.gpu
mm = 1e-3
U = 2.0 ** -53

# (x, y) of the 10 mm detector and whether it is turned once more before the snapshot.  y = 40 mm: the 15 mm bundle is still 12 mm wide, so
# rays pass the detector's edge; x = 3.5 mm at y = 120 mm cuts the 6 mm bundle; x = 30 mm records nothing; the others scan the focus.
PLACES = {1: [(0.0, 200.13 * mm)],
          3: [(0.0, 200.13 * mm), (30 * mm, 200 * mm), (0.0, 40 * mm)],
          8: [(0.0, 40 * mm), (3.5 * mm, 120 * mm), (0.0, 199 * mm), (0.0, 199.7 * mm), (30 * mm, 200 * mm), (0.0, 200.13 * mm), (0.0, 200.6 * mm),
              (0.0, 201 * mm)]}
RAYS = {1: 512, 3: 1024, 8: 700}


def _sweep(K, record_segments=True, fill_empty=False):
    """fill_empty: the place that records nothing is swapped for one just behind the focus"""
    system, cs, psfd, lam, D = airy_setup(num_rays=RAYS[K])

    def configure(c):
        x, y = PLACES[K][c]
        if fill_empty and x == 30 * mm:
            x, y = 0.2 * mm, 200.3 * mm
        bmo.translate_to3d(psfd, [x, y, 0.0])
        if c > 0:  # every configuration has its own orientation: turned about the axis and tipped, once more each time
            bmo.yrotate3d(psfd, np.radians(7))
            bmo.xrotate3d(psfd, np.radians(0.4))

    return bmo.solve_sweep(system, cs, K, configure, record_segments=record_segments), psfd


def _pose(sol, det, c):
    pos, ori = sol._poses[c][sol._slot(det)]
    return pos, ori[:, 0].copy(), ori[:, 2].copy()


@pytest.fixture(scope="module", params=[1, 3, 8])
def swept(request):
    K = request.param
    sol, psfd = _sweep(K)
    rows = [sol.detector_hits(psfd, c).copy() for c in range(K)]
    single = [abi.psf_stats(rows[c], *_pose(sol, psfd, c))[0] for c in range(K)]
    yield K, sol, psfd, rows, single
    sol.close()


def test_every_configuration_equals_the_single_call(swept):
    K, sol, psfd, rows, single = swept
    counts = [len(r) for r in rows]
    print("K = %d, rows per configuration: %s" % (K, counts))
    if K > 1:
        assert 0 in counts and len(set(counts)) >= 3, counts  # one records nothing, the counts are ragged
        poses = [_pose(sol, psfd, c) for c in range(K)]
        assert all(not np.array_equal(poses[0][1], p[1]) for p in poses[1:])
    st = sol.psf_stats(psfd)
    assert st.shape == (K, abi.PSF_STAT_N) and sol.readout_ms > 0
    for c in range(K):
        assert same_bits(st[c], single[c]), c
        if counts[c] == 0:
            assert st[c, pr.N] == 0 and np.isnan(st[c, 1:]).all()
        else:
            assert st[c, pr.N] == counts[c]
            assert pr.stat_violations(st[c], rows[c], *_pose(sol, psfd, c)) == [], c
    # a reference point per configuration, and one for all
    ref = np.column_stack([np.where(np.isnan(st[:, pr.CX]), 0.0, st[:, pr.CX]) + 1e-6, np.where(np.isnan(st[:, pr.CZ]), 0.0, st[:, pr.CZ]) - 2e-6])
    st_ref = sol.psf_stats(psfd, ref=ref)
    st_one = sol.psf_stats(psfd, ref=ref[0])
    for c in range(K):
        assert same_bits(st_ref[c], abi.psf_stats(rows[c], *_pose(sol, psfd, c), ref=ref[c])[0]), c
        assert same_bits(st_one[c], abi.psf_stats(rows[c], *_pose(sol, psfd, c), ref=ref[0])[0]), c
    full = [c for c in range(K) if counts[c]]
    assert (st_ref[full, pr.X_REF] == ref[full, 0]).all() and same_bits(st_ref[full][:, :pr.X_REF], st[full][:, :pr.X_REF])


def test_detector_only_result_reads_the_same(swept):
    K, sol, psfd, rows, single = swept
    sol0, psfd0 = _sweep(K, record_segments=False)
    try:
        assert same_bits(sol0.psf_stats(psfd0), sol.psf_stats(psfd))
    finally:
        sol0.close()


def test_device_window_reads_the_axes_of_the_statistics(swept):
    """window="device": bit for bit abi.psf_intensity on the axes psf_axes_from_stats gives from the single call's statistics.  Against
    window="host" the two fields are device sums at sample points that differ by the rounding of the window:
      * the host takes x_h from a matrix product; it and the header's expression are both within gamma_3 A of the exact dot product
        (A = max_h sum_i |(hit - origin)_i e_i|), so the two x_h differ by 2 gamma_3 A and so do their exact centroids; each computed centroid
        is within E_c of its exact one (any summation order: psf_stats_ref): the centres differ by D = 2 E_c + 2 gamma_3 A (the bounding-box
        centre by less).  The half-width follows the centre and the x_h: 2 D.  The limits centre -+ crop * half-width differ by
        (1 + 2 crop) D, plus the roundings of the product, the sum, linrange's three and the shift's one, each below u times
        M = max(|X_MIN|, |X_MAX|) + crop (X_MAX - X_MIN) + |shift|:   d_x = (1 + 2 crop) D + 8 u M,  d_z likewise;
      * |dF/dx| <= sum proj k |e1 . dir| <= k S, so the exact field moves by at most k S (d_x + d_z);
      * each device field is within B = psf_oracle_bound + psf_engine_bound of the exact field at its own points.
    dF = 2 B + k S (d_x + d_z), and |I_dev - I_host| <= 2 |F|max dF + dF^2 + 3 u Imax (the roundings of abs2)."""
    K, sol, psfd, rows, single = swept
    n = 16
    empty = [c for c in range(K) if len(rows[c]) == 0]
    if empty:
        for window in ("host", "device"):
            with pytest.raises(ValueError, match="configuration %d" % empty[0]):
                sol.psf_intensity(psfd, n=n, window=window)
        with pytest.raises(ValueError, match="window"):
            sol.psf_intensity(psfd, n=n, window="gpu")
        sol, psfd = _sweep(K, fill_empty=True)
        rows = [sol.detector_hits(psfd, c).copy() for c in range(K)]
        single = [abi.psf_stats(rows[c], *_pose(sol, psfd, c))[0] for c in range(K)]
    try:
        _check_windows(K, sol, psfd, rows, single, n)
    finally:
        if empty:
            sol.close()


def _check_windows(K, sol, psfd, rows, single, n):
    assert min(len(r) for r in rows) > 0
    for kw in (dict(crop_factor=3), dict(center="bbox", crop_factor=2, x0_shift=1e-7)):
        xs, zs, I, F = sol.psf_intensity(psfd, n=n, window="device", want_field=True, **kw)
        hx, hz, Ih, Fh = sol.psf_intensity(psfd, n=n, want_field=True, **kw)
        for c in range(K):
            pose = _pose(sol, psfd, c)
            ax, az = bmo.components.psf_axes_from_stats(single[c], n=n, **kw)
            assert np.array_equal(xs[c], ax) and np.array_equal(zs[c], az)
            I1, F1, _ = abi.psf_intensity(rows[c], *pose, ax, az, want_field=True)
            assert np.array_equal(I[c], I1) and np.array_equal(F[c], F1), (c, kw)
            # against the host window
            x, z = pr.local_xz(rows[c], *pose)
            ex = pr.exact_stats(x, z, x, rows[c][:, 7])
            _, e_cx, e_cz, _, _, _ = pr.sum_bounds(ex)
            loc = np.abs(rows[c][:, 0:3] - pose[0][None, :])
            g3 = 3 * U / (1 - 3 * U)
            a_x, a_z = (loc @ np.abs(pose[1])).max(), (loc @ np.abs(pose[2])).max()
            st = single[c]
            crop = kw.get("crop_factor", 1.0)
            m_x = max(abs(st[pr.X_MIN]), abs(st[pr.X_MAX])) + crop * (st[pr.X_MAX] - st[pr.X_MIN]) + abs(kw.get("x0_shift", 0.0))
            m_z = max(abs(st[pr.Z_MIN]), abs(st[pr.Z_MAX])) + crop * (st[pr.Z_MAX] - st[pr.Z_MIN]) + abs(kw.get("z0_shift", 0.0))
            d_x = (1 + 2 * crop) * (2 * float(e_cx) + 2 * g3 * a_x) + 8 * U * m_x
            d_z = (1 + 2 * crop) * (2 * float(e_cz) + 2 * g3 * a_z) + 8 * U * m_z
            assert np.abs(xs[c] - hx[c]).max() <= d_x and np.abs(zs[c] - hz[c]).max() <= d_z, (c, kw)
            S, k = float(rows[c][:, 7].sum()), float(rows[c][:, 8].max())
            B = rr.psf_oracle_bound(rows[c], rr.psf_max_phase(rows[c], *pose, ax, az)) + rr.psf_engine_bound(rows[c])
            dF = 2 * B + k * S * (d_x + d_z)
            fmax = max(np.abs(F[c]).max(), np.abs(Fh[c]).max())
            print("K = %d, c = %d: axes differ by (%.3g, %.3g) (bounds %.3g, %.3g); |F_dev - F_host| = %.3g S (bound %.3g S)"
                  % (K, c, np.abs(xs[c] - hx[c]).max(), np.abs(zs[c] - hz[c]).max(), d_x, d_z, np.abs(F[c] - Fh[c]).max() / S, dF / S))
            assert np.abs(F[c] - Fh[c]).max() <= dF, (c, kw)
            assert np.abs(I[c] - Ih[c]).max() <= 2 * fmax * dF + dF * dF + 3 * U * max(I[c].max(), Ih[c].max()), (c, kw)


def test_engine_solution_equals_the_sweep_form_with_one_configuration():
    sol, psfd = _sweep(1)
    try:
        pos, ori = sol._poses[0][sol._slot(psfd)]
        es = bmo.system.EngineSolution(sol.lib, sol._handle, sol.n_roots, 0)
        try:
            xs, zs, I = es.psf_intensity(sol._slot(psfd), pos, ori, n=20, crop_factor=4)
            assert same_bits(es.psf_stats(sol._slot(psfd), pos, ori), sol.psf_stats(psfd)[0])
        finally:
            es.handle = None  # the sweep solution owns the result
        sx, sz, sI = sol.psf_intensity(psfd, n=20, crop_factor=4, window="device")
        assert np.array_equal(xs, sx[0]) and np.array_equal(zs, sz[0]) and np.array_equal(I, sI[0])
    finally:
        sol.close()


def _raw(handle, slot, K, origin=True, stats=True):
    lib = abi.load_engine()
    dp = C.POINTER(C.c_double)
    K1 = max(K, 1)
    o, e1, e2 = np.zeros((K1, 3)), np.tile([1.0, 0, 0], (K1, 1)), np.tile([0, 0, 1.0], (K1, 1))
    st = np.zeros((K1, abi.PSF_STAT_N))
    return lib.bmo_psf_stats_sweep(handle, slot, K, o.ctypes.data_as(dp) if origin else None, e1.ctypes.data_as(dp), e2.ctypes.data_as(dp), None,
                                   st.ctypes.data_as(dp) if stats else None, None)


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
        assert _raw(sol._handle, ps, 3) == 0
        assert _raw(sol._handle, ss, 3) == -1  # a Spotdetector's slot
        assert "PSFDetector" in abi.load_engine().bmo_last_error().decode()
        for bad_k in (1, 2, 4, 0):
            assert _raw(sol._handle, ps, bad_k) == -1, bad_k
        assert _raw(sol._handle, 7, 3) == -1 and _raw(sol._handle, -1, 3) == -1
        assert _raw(sol._handle, ps, 3, origin=False) == -1 and _raw(sol._handle, ps, 3, stats=False) == -1
        with pytest.raises(RuntimeError, match="bmo_psf_stats_sweep"):
            sol.psf_stats(spot)
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
