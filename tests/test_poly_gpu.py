"""Polychromatic read-out on the GPU: the band split and the discovery against their numpy statements bit for bit, the combined stack against
bmo_psf_through_focus of every band and the left-to-right combination, its transform against the 40-digit transform of the image it returned,
and a two-colour solve through a dispersive singlet end to end.  Every bound is an existing derived one (tests/focus_ref.py, tests/mtf_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import focus_ref as fr
import mtf_ref as mr
import poly_ref as po
import scenes
from test_focus_gpu import MP, _axes, _oblique, _solve
from test_mtf_gpu import FREQS5

pytestmark = pytest.mark.gpu

mm = 1e-3
KS3 = np.array([po.wave_number(l) for l in po.WAVELENGTHS])


def _download(ptr, count):
    """count rows of 9 doubles from the device pointer ptr"""
    out = np.zeros((count, 9))
    if count:
        hip = C.CDLL("libamdhip64.so")
        assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return out


def _check_split(bands, rows, ks, unmatched):
    """Every band of the handle equals the masked rows, bit for bit and in order."""
    want, want_unmatched = po.band_split(rows, ks)
    assert unmatched == want_unmatched
    assert np.array_equal(po.bits(bands.ks), po.bits(np.asarray(ks, dtype=np.float64))) and bands.unmatched == unmatched
    assert bands.counts.tolist() == [len(w) for w in want] and bands.n_rows == sum(len(w) for w in want)
    for b, w in enumerate(want):
        ptr, cnt = bands.rows(b)
        assert cnt == len(w) and ptr != 0
        assert np.array_equal(po.bits(_download(ptr, cnt)), po.bits(w)), b


def _check_both_forms(rows, ks, unmatched_listed):
    with abi.psf_bands(rows, ks=ks) as b:
        _check_split(b, rows, ks, unmatched_listed)
    dk, dc, dn = po.discover(rows)
    with abi.psf_bands(rows) as b:
        assert b.counts.tolist() == dc.tolist()
        _check_split(b, rows, dk, dn)


# ------------------------------------------------------------------------------------------------ split and discovery
def test_split_and_discovery_main_case():
    """H = 600: two full tiles and a ragged one of 88 rows.  Three bands in an irregular interleave, a fourth listed band without a row, 7 rows
    of an unlisted key and 2 rows with a NaN key."""
    rng = np.random.Generator(np.random.PCG64(11))
    band = rng.integers(0, 3, 600)
    odd = rng.permutation(600)[:9]
    band[odd[:7]], band[odd[7:]] = 4, 5
    listed = [KS3[1], KS3[0], KS3[2], 1.25e7]  # the caller's order, not ascending; the last has no row
    rows = po.synthetic_rows(band, listed + [9.5e6, np.nan])
    assert min(np.bincount(band, minlength=6)[:3]) > 150 and (band[:256] != band[0]).any()
    with abi.psf_bands(rows, ks=listed, want_ms=True)[0] as b:
        _check_split(b, rows, listed, 9)
        assert b.counts[3] == 0 and b.device == 0 and len(b) == 4
    dk, dc, dn = po.discover(rows)
    assert len(dk) == 4 and dn == 2 and dc.sum() == 598
    bands, ms = abi.psf_bands(rows, want_ms=True)
    with bands as b:
        assert ms > 0 and b.counts.tolist() == dc.tolist()
        _check_split(b, rows, dk, 2)


@pytest.mark.parametrize("H", [0, 1, 256, 257])
def test_split_edge_row_counts(H):
    """No rows, one row, exactly one tile, one tile and a row; two bands row by row."""
    rows = po.synthetic_rows(np.arange(H) % 2, KS3[:2])
    _check_both_forms(rows, [KS3[1], KS3[0]], 0)
    if H == 0:
        with abi.psf_bands(rows) as b:
            assert len(b) == 0 and b.n_rows == 0 and b.unmatched == 0


def test_split_waves_that_agree_and_waves_that_do_not():
    """All rows in one band; 64 bands with row i in band i % 64, so that every lane of a wave disagrees with every other; the same rows
    sorted by band, so that every wave but those at a boundary agrees."""
    ks64 = 1e7 + 1e3 * np.arange(64.0)[::-1]  # descending: the caller's order is kept
    one = po.synthetic_rows(np.zeros(600, dtype=np.int64), KS3[:1])
    _check_both_forms(one, [KS3[0]], 0)
    spread = po.synthetic_rows(np.arange(600) % 64, ks64)
    _check_both_forms(spread, ks64, 0)
    ordered = spread[np.argsort(spread[:, 8], kind="stable")]
    _check_both_forms(ordered, ks64, 0)
    with abi.psf_bands(spread, ks=ks64[:3]) as b:  # the other 61 keys are unmatched
        _check_split(b, spread, ks64[:3], 600 - sum(len(range(q, 600, 64)) for q in range(3)))


def test_split_refusals():
    rows65 = po.synthetic_rows(np.arange(130) % 65, 1e7 + np.arange(65.0))
    with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-6\)"):
        abi.psf_bands(rows65)
    with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-6\)"):
        abi.psf_bands(rows65, ks=1e7 + np.arange(65.0))
    with abi.psf_bands(rows65, ks=1e7 + np.arange(64.0)) as b:  # 64 of them are legal
        assert b.unmatched == 2 and b.counts.tolist() == [2] * 64
    for ks in ([1.0, 1.0], [1.0, np.nan], [np.inf, 1.0]):
        with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-1\)"):
            abi.psf_bands(rows65, ks=ks)
    with abi.psf_bands(rows65[:4]) as b:
        with pytest.raises(IndexError):
            b.rows(4)
        assert b.lib.bmo_psf_bands_get(b.handle, 4, None, None, None) == -1 and b.lib.bmo_psf_bands_get(b.handle, -1, None, None, None) == -1


# ------------------------------------------------------------------------------------------------ the polychromatic stack
@pytest.fixture(scope="module")
def colour600():
    """tilted_psf_case(600) with column 8 rewritten to three wavelengths: (rows, pose, o)."""
    rows, pose, o = _solve(600)
    rows = po.recolour(rows)
    assert min(int((rows[:, 8] == k).sum()) for k in KS3) > 150
    return rows, pose, o


@pytest.mark.parametrize("n", [5, 17])
def test_poly_stack_is_the_combination_of_the_band_stacks(colour600, n):
    """Every I_b equals bmo_psf_through_focus of the band's host rows, the sum the numpy left-to-right combination, both as uint64 views; a
    zero coefficient and a band without rows; one band with coefficient 1 is the monochromatic call; and the incoherent sum is not the
    coherent one."""
    rows, pose, o = colour600
    M = MP + 1
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    ks = [KS3[2], 1.1e7, KS3[0], KS3[1]]  # the caller's order; the second band has no row
    want_b = [abi.psf_through_focus(rows[rows[:, 8] == k], *pose, d, xs, zs)[0] for k in ks]
    assert not want_b[1].any()
    with abi.psf_bands(rows, ks=ks) as b:
        for coeffs in ([0.7, 2.0, 1.3, 0.45], [1.0, 1.0, 0.0, -0.25]):
            I, I_b, ms = abi.psf_poly_through_focus(b, *pose, d, xs, zs, coeffs, want_bands=True)
            assert I.shape == (M, n, n) and I_b.shape == (4, M, n, n) and ms > 0
            for q in range(4):
                assert np.array_equal(po.bits(I_b[q]), po.bits(want_b[q])), q
            assert np.array_equal(po.bits(I), po.bits(po.combine(coeffs, want_b)))
            assert np.array_equal(po.bits(I), po.bits(abi.psf_poly_through_focus(b, *pose, d, xs, zs, coeffs)[0]))
    with abi.psf_bands(rows, ks=[KS3[1]]) as b:
        I1, _, _ = abi.psf_poly_through_focus(b, *pose, d, xs, zs, [1.0])
        assert np.array_equal(po.bits(I1), po.bits(abi.psf_through_focus(rows[rows[:, 8] == KS3[1]], *pose, d, xs, zs)[0]))
    with abi.psf_bands(rows) as b:  # discovery: ascending
        assert np.array_equal(b.ks, np.sort(KS3))
        I, _, _ = abi.psf_poly_through_focus(b, *pose, d, xs, zs, [1.0, 1.0, 1.0])
    I_c, F_c, _ = abi.psf_through_focus(rows, *pose, d, xs, zs, want_field=True)
    f_abs = np.abs(F_c).max() * (1 + 1e-6)
    bound = max(fr.stack_bound(rows, *pose, d[m], xs, zs, f_abs) for m in range(M))
    i_bound = 2 * f_abs * np.sqrt(2) * bound * (1 + 1e-6) + 8 * fr.U * f_abs ** 2  # what a field inside `bound` moves its abs2 by
    print("n = %d: incoherent - coherent %.3e, bound of the coherent stack %.3e" % (n, np.abs(I - I_c).max(), i_bound))
    assert np.abs(I - I_c).max() > 1e6 * i_bound


def test_poly_stack_without_bands_or_rows(colour600):
    rows, pose, o = colour600
    xs, zs = _axes(rows, pose, o, 5)
    d = _oblique(pose, 3)
    with abi.psf_bands(rows[:0]) as b:
        I, I_b, _ = abi.psf_poly_through_focus(b, *pose, d, xs, zs, [], want_bands=True)
        assert I.shape == (3, 5, 5) and not I.any() and I_b.shape == (0, 3, 5, 5)
        mtf, otf, sums, img, _ = abi.psf_poly_otf(b, *pose, d, xs, zs, [], FREQS5, want_intensity=True)
        assert np.isnan(mtf).all() and not otf.any() and not sums.any() and not img.any()
    with abi.psf_bands(rows, ks=[1.1e7, 1.2e7]) as b:  # two bands, no row in either
        assert b.unmatched == 600
        I, _, _ = abi.psf_poly_through_focus(b, *pose, d, xs, zs, [1.0, 2.0])
        assert not I.any()
        assert np.isnan(abi.psf_poly_otf(b, *pose, d, xs, zs, [1.0, 2.0], FREQS5)[0]).all()
        for bad in ([1.0, np.nan], [np.inf, 1.0]):
            with pytest.raises(RuntimeError, match=r"bmo_psf_poly_through_focus failed \(-1\)"):
                abi.psf_poly_through_focus(b, *pose, d, xs, zs, bad)
        with pytest.raises(RuntimeError, match=r"bmo_psf_poly_otf failed \(-1\)"):
            abi.psf_poly_otf(b, *pose, d, xs, zs, [1.0, 2.0], [[np.nan, 0.0]])
        with pytest.raises(ValueError, match="one coefficient per band"):
            abi.psf_poly_through_focus(b, *pose, d, xs, zs, [1.0])


# ------------------------------------------------------------------------------------------------ the polychromatic OTF
@pytest.mark.parametrize("n,M", [(5, 1), (17, MP + 1)])
def test_poly_otf_is_the_transform_of_the_combined_stack(colour600, n, M):
    rows, pose, o = colour600
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    pitch = max(np.abs(np.diff(xs)).max(), np.abs(np.diff(zs)).max())
    freqs = FREQS5 / np.abs(FREQS5).max() * 0.45 / pitch
    bmo.components.mtf_check_pitch(xs, zs, freqs)
    with abi.psf_bands(rows) as b:
        S = np.array([rows[rows[:, 8] == k, 7].sum() for k in b.ks])
        coeffs = bmo.components.poly_coefficients([1.0, 0.7, 0.4], S)
        mtf, otf, sums, I, ms = abi.psf_poly_otf(b, *pose, d, xs, zs, coeffs, freqs, want_intensity=True)
        assert mtf.shape == otf.shape == (M, 5) and I.shape == (M, n, n) and ms > 0
        assert np.array_equal(po.bits(I), po.bits(abi.psf_poly_through_focus(b, *pose, d, xs, zs, coeffs)[0]))
    for m in sorted({0, M - 1, M // 2}):
        T, total = mr.otf_exact(I[m], xs, zs, freqs)
        assert abs(sums[m] - total) <= fr.gamma(2 * n) * total
        for q in range(len(freqs)):
            bound = mr.otf_bound(total, xs, zs, freqs[q], abs(T[q]))
            err = max(abs(otf[m, q].real - T[q].real), abs(otf[m, q].imag - T[q].imag))
            want = abs(T[q]) / total
            print("plane %d f %d: component error %.3e bound %.3e; MTF %.6f error %.2e" % (m, q, err, bound, mtf[m, q], abs(mtf[m, q] - want)))
            assert err <= bound < 1e-12 * total, (m, q, err, bound)
            assert abs(mtf[m, q] - want) <= mr.mtf_bound(bound, total, want, 2 * n) + fr.U * want, (m, q)
        assert 0 < mtf[m].max() < 1.0


# ------------------------------------------------------------------------------------------------ end to end
LAM_GREEN, LAM_RED = 546.1e-9, 656.3e-9
OFFSETS = np.linspace(-4 * mm, 4 * mm, 33)
EXACT = [0, 16, 32]  # the planes held to the 40-digit statistics


def _singlet(lams):
    """A plano-convex singlet of the microscope tutorial's N-BK7 and a PSFDetector near its foci; 300 rays per colour, interleaved ray by
    ray in one bundle: (system, detector, bundle)."""
    lens = bmo.SphericalLens(100 * mm, np.inf, 3 * mm, 25.4 * mm, bmo.DiscreteRefractiveIndex([LAM_GREEN, LAM_RED], [1.51872, 1.51432]))
    psfd = bmo.PSFDetector(10 * mm)
    bmo.translate3d(psfd, [0, 194.5 * mm, 0])
    one = [scenes.disc_bundle(300, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=10 * mm, lam=lam, jitter=0.0) for lam in lams]
    planes = np.empty((one[0].planes.shape[0], 300 * len(lams)))
    for q, b in enumerate(one):
        planes[:, q::len(lams)] = b.planes
    return bmo.System([lens, psfd]), psfd, bmo.RayBundle(one[0].kind, planes)


def _solve_singlet(lams):
    system, psfd, bundle = _singlet(lams)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    rows_view, sol = bmo.system._engine_solve(scene, bundle, 100, None)
    rows = rows_view.detector_hits(0).copy()
    return rows, sol, np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)


def _lex(rows):
    return rows[np.lexsort(rows.T[::-1])]


def test_two_colours_through_a_dispersive_singlet():
    rows, sol, pos, o = _solve_singlet([LAM_GREEN, LAM_RED])
    e1, e2, axis = o[:, 0], o[:, 2], o[:, 1]
    k_green, k_red = po.wave_number(LAM_GREEN), po.wave_number(LAM_RED)
    bands = sol.psf_bands(0)
    try:
        assert sol.readout_ms > 0
        # discovery: ascending k, so red first; 300 rows each, the keys bit for bit what the engine writes
        assert np.array_equal(po.bits(bands.ks), po.bits(np.array([k_red, k_green]))) and bands.counts.tolist() == [300, 300] and bands.unmatched == 0
        # resident rows equal host rows: the same handle from the copied rows
        with abi.psf_bands(rows) as host:
            assert np.array_equal(po.bits(host.ks), po.bits(bands.ks))
            for b in range(2):
                assert np.array_equal(po.bits(_download(*bands.rows(b))), po.bits(_download(*host.rows(b))))
        _check_split(bands, rows, bands.ks, 0)
        # the handle outlives the result it was built from
        ks, st_sol, focus_sol, _, cen_sol, plane_sol = sol.psf_chromatic_focus(0, pos, o, OFFSETS)
        sol.free()
        _check_split(bands, rows, bands.ks, 0)
        (st, focus, rms, cen, plane), ms = bmo.components.chromatic_focus_of(bands, pos, o, OFFSETS)
        assert ms > 0 and np.array_equal(po.bits(st), po.bits(st_sol)) and np.array_equal(focus, focus_sol) and plane == plane_sol
        band_rows = po.band_split(rows, bands.ks)[0]
        exact = [fr.focus_stats_exact(r, pos, e1, e2, axis, OFFSETS[EXACT]) for r in band_rows]
        for b in range(2):
            direct = abi.psf_focus_stats(band_rows[b], pos, e1, e2, axis, OFFSETS)[0]
            assert np.array_equal(po.bits(st[b]), po.bits(direct))  # the pointer reads as the host rows do
            for m, ex in zip(EXACT, exact[b]):
                assert fr.stat_violations(st[b, m], ex) == [], (b, m)
        # longitudinal colour: red (band 0) focuses further from the lens, which sits at the origin, than green (band 1)
        dist = np.linalg.norm(pos[None, :] + focus[:, None] * axis[None, :], axis=1)
        print("best focus: red %+.4e m, green %+.4e m along local y; %.6f / %.6f m from the lens; rms there %.3e / %.3e m"
              % (focus[0], focus[1], dist[0], dist[1], rms[0], rms[1]))
        assert (OFFSETS[1] < focus).all() and (focus < OFFSETS[-2]).all() and dist[0] - dist[1] > 1 * mm
        assert np.isfinite(cen).all()
    finally:
        bands.close()
        sol.free()
    # every colour solved alone: the same rows, and the same focus curve inside both bounds
    for b, lam in ((0, LAM_RED), (1, LAM_GREEN)):
        alone, sol1, pos1, o1 = _solve_singlet([lam])
        sol1.free()
        assert np.array_equal(pos1, pos) and np.array_equal(o1, o) and len(alone) == 300
        assert np.array_equal(po.bits(_lex(alone)), po.bits(_lex(band_rows[b]))), lam
        st1 = abi.psf_focus_stats(alone, pos, e1, e2, axis, OFFSETS[EXACT])[0]
        ex1 = fr.focus_stats_exact(alone, pos, e1, e2, axis, OFFSETS[EXACT])
        for q, m in enumerate(EXACT):
            b_band, b_alone = fr.stat_bounds(exact[b][q]), fr.stat_bounds(ex1[q])
            for col in (fr.CX, fr.CZ, fr.RMS_R, fr.MAX_R, fr.HWX, fr.HWZ):
                assert abs(st[b, m, col] - st1[q, col]) <= b_band[col] + b_alone[col], (lam, m, col)


def test_detector_and_solution_read_the_same_polychromatic_stack_and_mtf():
    """PSFDetector.poly_through_focus / poly_mtf on the copied rows and EngineSolution's on the resident ones, bit for bit; the window comes
    from the statistics of all rows, the half-width of the MTF grid from the smallest wave number."""
    rows, sol, pos, o = _solve_singlet([LAM_GREEN, LAM_RED])
    psfd = bmo.PSFDetector(10 * mm)
    psfd.data, psfd.position, psfd.orientation = rows, (lambda: pos), (lambda: o)
    offsets = [-1.0 * mm, 0.0, 1.0 * mm]
    try:
        got = sol.psf_poly_through_focus(0, pos, o, offsets, weights=[1.0, 0.5], n=9, want_bands=True)
        want = psfd.poly_through_focus(offsets, weights=[1.0, 0.5], n=9, want_bands=True)
        assert sol.readout_ms > 0 and len(got) == 8
        for a, b in zip(got, want):
            assert np.array_equal(po.bits(a), po.bits(b))
        xs, zs, d, I, st, ks, coeffs, I_b = got
        assert I.shape == (3, 9, 9) and I_b.shape == (2, 3, 9, 9) and np.array_equal(po.bits(I), po.bits(po.combine(coeffs, I_b)))
        S = np.array([rows[rows[:, 8] == k, 7].sum() for k in ks])
        assert np.abs(coeffs * S * S / np.array([1.0, 0.5]) - 1).max() < 1e-12 and (I >= 0).all() and I.max() > 0
        assert np.array_equal(st, abi.psf_focus_stats(rows, pos, o[:, 0], o[:, 2], o[:, 1], offsets)[0])  # the window: all rows
        freqs = bmo.components.mtf_frequencies(2e4, 5)
        got = sol.psf_poly_mtf(0, pos, o, freqs, offsets=offsets[:2])
        want = psfd.poly_mtf(freqs, offsets=offsets[:2])
        for a, b in zip(got, want):
            assert np.array_equal(po.bits(a), po.bits(b))
        assert got[0].shape == (2, 5) and np.abs(got[0][:, 0] - 1.0).max() < 1e-12 and np.isfinite(got[0]).all() and (got[0] <= 1 + 1e-12).all()
        for slot in (-1, 1):
            with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-1\)"):
                sol.psf_bands(slot)
    finally:
        sol.free()
