"""MTF read-out of sweeps on the GPU (include/bmo_sweep_readout.h): bmo_psf_geo_otf_sweep and bmo_psf_otf_sweep equal, configuration by
configuration and bit for bit in every output, bmo_psf_geo_otf and bmo_psf_otf on that configuration's rows with its pose, planes, centres
and axes; SweepSolution.psf_mtf equals components.psf_mtf driven by single calls on the host rows, given the sweep's n and the
configuration's half-width.

Scenes and helpers: test_focus_sweep_gpu.py.  Shapes: M = 1, 9, 17 planes (9 crosses the 8-plane chunks of the geometric MTF), n = 5 and
17, nf = 1 and 33 frequencies (frequency 0 included; 33 crosses a block of 32 frequencies at 8 planes per chunk), centres given and NULL."""
import numpy as np
import pytest

from bmo_amd import abi
from bmo_amd import components as cp
import focus_ref as fr
from test_focus_sweep_gpu import (GRIDS, PLANES, check_a_gaussian_result_is_unsupported, check_common_refusals, check_shape_of_the_scene, grid_axes, make_sweep,
                                  planes, poses, raw, refusal_sweep)
from test_psf_stats import same_bits
from test_psf_stats_sweep_gpu import _pose

pytestmark = pytest.mark.gpu
mm = 1e-3
FREQS = {1: np.zeros((1, 2)), 33: cp.mtf_frequencies(3e4, 33, azimuth_deg=30)}


@pytest.fixture(scope="module", params=[1, 3, 8, "big"])
def swept(request):
    key = request.param
    sol, psfd = make_sweep(key)
    rows = [sol.detector_hits(psfd, c).copy() for c in range(sol.n)]
    yield key, sol, psfd, rows
    sol.close()


def _same_otf(got, want, what):
    """(mtf, otf, sums) of one configuration"""
    assert same_bits(got[0], want[0]) and same_bits(got[1].real, want[1].real) and same_bits(got[1].imag, want[1].imag) and same_bits(got[2], want[2]), what


def _empty_otf(got):
    return np.isnan(got[0]).all() and not got[1].any() and not got[2].any()


def test_every_configuration_equals_the_single_geometric_call(swept):
    key, sol, psfd, rows = swept
    K = sol.n
    counts = check_shape_of_the_scene(key, rows)
    slot, pos, e1s, e2s, _ = poses(sol, psfd)
    assert FREQS[33][0].tolist() == [0.0, 0.0]
    for M in PLANES:
        axes, off, _, cen = planes(sol, psfd, rows, M)
        for nf, fq in FREQS.items():
            for centers in (None, cen):
                got = abi.psf_geo_otf_sweep(sol._handle, slot, K, pos, e1s, e2s, axes, off, fq, centers=centers)
                assert got[0].shape == (K, M, nf) and got[1].shape == (K, M, nf) and got[2].shape == (K, M) and got[3] > 0
                for c in range(K):
                    want = abi.psf_geo_otf(rows[c], *_pose(sol, psfd, c), axes[c], off[c], fq, centers=None if centers is None else centers[c])
                    _same_otf([g[c] for g in got[:3]], want, (M, nf, c, centers is None))
                    if counts[c] == 0:
                        assert _empty_otf([g[c] for g in got[:3]])
                    else:
                        assert np.isfinite(got[0][c]).all() and np.abs(got[0][c][:, 0] - 1.0).max() < 1e-12  # |T(0)| / T(0)
        st = abi.psf_focus_stats_sweep(sol._handle, slot, K, pos, e1s, e2s, axes, off)[0]
        full = [c for c in range(K) if counts[c]]
        assert same_bits(got[2][full], st[full][:, :, fr.S])  # S is the focus statistics' sum, bit for bit


def test_every_configuration_equals_the_single_diffraction_call(swept):
    key, sol, psfd, rows = swept
    K = sol.n
    counts = [len(r) for r in rows]
    slot, pos, e1s, e2s, _ = poses(sol, psfd)
    for M in PLANES:
        _, _, disp, _ = planes(sol, psfd, rows, M)
        for n in GRIDS:
            xs, zs = grid_axes(rows, n)
            stack = abi.psf_through_focus_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs)[0]
            for nf, fq in FREQS.items():
                got = abi.psf_otf_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs, fq, want_intensity=True)
                plain = abi.psf_otf_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs, fq)
                assert got[0].shape == (K, M, nf) and got[3].shape == (K, M, n, n) and got[4] > 0 and plain[3] is None
                assert same_bits(got[3], stack)  # the images are those of bmo_psf_through_focus_sweep
                for a, b in zip(got[:3], plain[:3]):
                    assert same_bits(a.real, b.real) and same_bits(a.imag, b.imag)
                for c in range(K):
                    want = abi.psf_otf(rows[c], *_pose(sol, psfd, c), disp[c], xs[c], zs[c], fq, want_intensity=True)
                    _same_otf([g[c] for g in got[:3]], want, (M, n, nf, c))
                    assert same_bits(got[3][c], want[3]), (M, n, nf, c)
                    if counts[c] == 0:
                        assert _empty_otf([g[c] for g in got[:3]]) and not got[3][c].any()
                    else:
                        assert np.isfinite(got[0][c]).all() and (got[2][c] > 0).all()


def _window(rows, pose):
    """(k_max, rho, n_rows) of one configuration from single calls: what EngineSolution.psf_mtf hands components.mtf_window"""
    st, info = abi.psf_stats(rows, *pose)[0], abi.psf_zernike(rows, *pose, order=0)[1]
    return st[abi.PSF_K_MAX], info[abi.ZERN_RHO], int(st[abi.PSF_N])


def _single_mtf(rows, pose, ori, freqs, offsets, **kw):
    """components.psf_mtf driven by single calls on host rows"""
    return cp.psf_mtf(lambda ax, off: abi.psf_focus_stats(rows, *pose, ax, off)[0],
                      lambda ax, off, fq, cen: abi.psf_geo_otf(rows, *pose, ax, off, fq, centers=cen)[:3],
                      lambda d, xs, zs, fq: abi.psf_otf(rows, *pose, d, xs, zs, fq)[:3], lambda: _window(rows, pose), ori, freqs, offsets=offsets, **kw)


def test_the_python_method_equals_the_single_path(swept):
    key, sol, psfd, rows = swept
    K = sol.n
    offsets = np.linspace(-0.3 * mm, 0.3 * mm, 3)
    ori = [np.asarray(sol._poses[c][sol._slot(psfd)][1], dtype=np.float64) for c in range(K)]
    full = [c for c in range(K) if len(rows[c])]
    # frequencies up to 0.15 of the cutoff of the first configuration: a grid of a few dozen points per axis
    k0, rho0, _ = _window(rows[full[0]], _pose(sol, psfd, full[0]))
    freqs = cp.mtf_frequencies(0.15 * cp.mtf_cutoff(k0, rho0), 4, azimuth_deg=20)
    f_max = float(np.abs(freqs).max())
    for follow in ("centroid", None):
        geo = sol.psf_mtf(psfd, freqs, offsets=offsets, kind="geometric", follow=follow)
        assert geo[0].shape == (K, 3, 4) and geo[3].shape == (K, 3, 12) and sol.readout_ms > 0
        for c in range(K):
            if c in full:
                want = _single_mtf(rows[c], _pose(sol, psfd, c), ori[c], freqs, offsets, kind="geometric", follow=follow)
                _same_otf([g[c] for g in geo[:3]], want[:3], (c, follow))
                assert same_bits(geo[3][c], want[3])
            else:
                assert _empty_otf([g[c] for g in geo[:3]]) and (geo[3][c, :, fr.N] == 0).all()
    # diffraction: the sweep takes the largest n any configuration's window asks for, every configuration keeps its own half-width
    grids = {c: cp.mtf_window(*_window(rows[c], _pose(sol, psfd, c)), f_max) for c in full}
    n = max(g[1] for g in grids.values())
    print("%r: n = %d, half-widths %s" % (key, n, {c: "%.3g" % g[0] for c, g in grids.items()}))
    for kw, single_kw in ((dict(), lambda c: dict(n=n, half_width=grids[c][0])), (dict(half_width=2e-5, follow=None), lambda c: dict(half_width=2e-5, follow=None)),
                          (dict(n=21, half_width=(1.5e-5, 2e-5)), lambda c: dict(n=21, half_width=(1.5e-5, 2e-5)))):
        got = sol.psf_mtf(psfd, freqs, offsets=offsets, **kw)
        assert got[0].shape == (K, 3, 4) and sol.readout_ms > 0
        for c in range(K):
            if c in full:
                want = _single_mtf(rows[c], _pose(sol, psfd, c), ori[c], freqs, offsets, **single_kw(c))
                _same_otf([g[c] for g in got[:3]], want[:3], (c, kw))
                assert same_bits(got[3][c], want[3])
            else:
                assert _empty_otf([g[c] for g in got[:3]]) and (got[3][c, :, fr.N] == 0).all() and np.isnan(got[3][c, :, 1:]).all()


def test_detector_only_result_reads_the_same(swept):
    key, sol, psfd, rows = swept
    sol0, psfd0 = make_sweep(key, record_segments=False)
    freqs = cp.mtf_frequencies(2e4, 3)
    try:
        for kw in (dict(kind="geometric"), dict(n=9, half_width=2e-5)):
            for a, b in zip(sol0.psf_mtf(psfd0, freqs, offsets=(-1e-4, 0.0, 1e-4), **kw), sol.psf_mtf(psfd, freqs, offsets=(-1e-4, 0.0, 1e-4), **kw)):
                assert same_bits(a.real, b.real) and same_bits(a.imag, b.imag), kw
    finally:
        sol0.close()


def test_refusals():
    check_common_refusals("bmo_psf_geo_otf_sweep", ("origins", "e1s", "e2s", "axes", "offsets", "freqs", "otf", "mtf", "sums"), ("n_planes", "n_freqs"))
    check_common_refusals("bmo_psf_otf_sweep", ("origins", "e1s", "e2s", "displacements", "xs", "zs", "freqs", "otf", "mtf", "sums"), ("n_planes", "n", "n_freqs"))
    sol, psfd, spot = refusal_sweep()
    try:
        ps = sol._slot(psfd)
        err = lambda: abi.load_engine().bmo_last_error().decode()  # noqa: E731
        assert raw("bmo_psf_geo_otf_sweep", sol._handle, ps, 3, null="centers") == 0 and raw("bmo_psf_otf_sweep", sol._handle, ps, 3, null="out_intensity") == 0
        for entry in ("bmo_psf_geo_otf_sweep", "bmo_psf_otf_sweep"):
            for bad in (np.nan, np.inf, -np.inf):
                assert raw(entry, sol._handle, ps, 3, freqs=[[1e3, 0.0], [0.0, bad]]) == -1 and "finite" in err(), (entry, bad)
        with pytest.raises(RuntimeError, match="bmo_psf_focus_stats_sweep"):
            sol.psf_mtf(spot, [[1e3, 0.0]])
        with pytest.raises(ValueError, match="finite"):
            sol.psf_mtf(psfd, [[np.nan, 0.0]])
        with pytest.raises(ValueError, match="kind"):
            sol.psf_mtf(psfd, [[1e3, 0.0]], kind="wave")
        with pytest.raises(ValueError, match="alias"):
            sol.psf_mtf(psfd, [[1e6, 0.0]], n=4, half_width=1e-4)
    finally:
        sol.close()


def test_a_gaussian_result_is_unsupported():
    check_a_gaussian_result_is_unsupported("bmo_psf_geo_otf_sweep")
    check_a_gaussian_result_is_unsupported("bmo_psf_otf_sweep")
