"""MTF read-out on the GPU: bmo_psf_geo_otf against the 40-digit transfer function of the propagated rows, bmo_psf_otf against the 40-digit
transform of the image the same call returned, the bit-for-bit identities both promise, and the Python layer.  Every bound is derived in
tests/mtf_ref.py; nothing is fitted."""
import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import focus_ref as fr
import mtf_ref as mr
import readout_ref as rr
import spot_ref as sr
from test_focus_gpu import MP, _axes, _oblique, _solve

pytestmark = pytest.mark.gpu

mm = 1e-3
H_ALL = 5000
FREQS5 = np.array([[3e4, -2e4], [-1.5e4, 2.5e4], [5e3, 4e4], [4.5e4, 1e3], [-7e3, -9e3]])  # cycles/m, no zero component


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.fixture(scope="module")
def case():
    """tilted_psf_case at 5000 rays solved once; a test of fewer rows takes the first of them."""
    ns, per = sr.spot_splits(H_ALL)
    assert ns == 3 and (H_ALL - 2 * per) % 256 != 0  # three splits, the third ends in a ragged tile
    rows, pose, o = _solve(H_ALL)
    assert np.all(np.abs(pose[1]) > 1e-3) and np.all(np.abs(pose[2]) > 1e-3) and (rows[:, 3:6] != 0).all()
    return rows, pose, o


def _axis(pose):
    return np.cross(pose[1], pose[2]) + 0.05 * pose[1] - 0.03 * pose[2]  # oblique to the planes, no zero component


def _check_geo(rows, pose, axis, offsets, centers, freqs, got, planes, fsel):
    """The (planes x fsel) entries of got = (mtf, otf, sums) against the exact transfer function, inside the derived bounds."""
    mtf, otf, sums = got
    cen = None if centers is None else np.asarray(centers)[planes]
    T, S, scales = mr.geo_otf_exact(rows, *pose, axis, np.asarray(offsets)[planes], np.asarray(freqs)[fsel], centers=cen)
    exact = fr.focus_stats_exact(rows, *pose, axis, np.asarray(offsets)[planes])
    H = len(rows)
    for a, m in enumerate(planes):
        assert abs(sums[m] - S) <= fr.gamma(max(H - 1, 1)) * S
        for b, q in enumerate(fsel):
            bound = mr.geo_bound(H, S, mr.e_row(exact[a]), scales[a], freqs[q], abs(T[a, b]))
            err = max(abs(otf[m, q].real - T[a, b].real), abs(otf[m, q].imag - T[a, b].imag))
            want = abs(T[a, b]) / S
            mb = mr.mtf_bound(bound, S, want, max(H - 1, 1)) + fr.U * want
            print("H = %d plane %d f = (%g, %g): component error %.3e bound %.3e; MTF %.6f error %.2e bound %.2e"
                  % (H, m, freqs[q][0], freqs[q][1], err, bound, mtf[m, q], abs(mtf[m, q] - want), mb))
            assert err <= bound < 1e-9 * S, (m, q, err, bound)
            assert abs(mtf[m, q] - want) <= mb, (m, q)


def test_geometric_against_the_exact_transfer_function(case):
    """H = 600, three planes along an oblique axis, five frequencies without a zero component, the phase counted from each plane's centroid."""
    rows, pose, o = case
    rows, axis, offsets = rows[:600], _axis(pose), np.array([-0.4 * mm, 0.07 * mm, 0.5 * mm])
    st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
    centers = st[:, [fr.CX, fr.CZ]]
    got = abi.psf_geo_otf(rows, *pose, axis, offsets, FREQS5, centers=centers)
    assert got[0].shape == got[1].shape == (3, 5) and got[2].shape == (3,) and got[3] > 0
    _check_geo(rows, pose, axis, offsets, centers, FREQS5, got[:3], [0, 1, 2], [0, 1, 2, 3, 4])
    assert np.array_equal(_bits(got[2]), _bits(st[:, fr.S]))
    assert np.abs(got[0][0] - got[0][1]).max() > 1e-3  # the planes differ by far more than a bound
    # without centres the phase is counted from the plane's origin: another phase, the same modulus inside both bounds
    bare = abi.psf_geo_otf(rows, *pose, axis, offsets, FREQS5)
    _check_geo(rows, pose, axis, offsets, None, FREQS5, bare[:3], [1], [0, 4])
    assert np.abs(bare[1] - got[1]).max() > 1e-3 * got[2][0]


@pytest.mark.parametrize("H", [0, 1, 256, 257])
def test_geometric_edge_row_counts(case, H):
    """No rows, one row, exactly one tile, one tile and a row."""
    rows, pose, o = case
    rows, axis, offsets, freqs = rows[:H], _axis(pose), np.array([0.0, 0.3 * mm]), FREQS5[:3]
    mtf, otf, sums, _ = abi.psf_geo_otf(rows, *pose, axis, offsets, freqs)
    assert mtf.shape == (2, 3)
    if H == 0:
        assert not otf.any() and not sums.any() and np.isnan(mtf).all()
        return
    _check_geo(rows, pose, axis, offsets, None, freqs, (mtf, otf, sums), [0, 1], [0, 1, 2])
    if H == 1:
        assert np.abs(mtf - 1.0).max() <= 32 * fr.U  # |cis| of one row: two components at 4 ulp, the squares, the root, the quotient


def test_geometric_three_splits_the_third_ragged(case):
    """H = 5000: splits of 1792, 1792 and 1416 rows; nine planes (a second, partial chunk) and seven frequencies, 2 x 2 of them against the
    exact values; S equals the focus statistics' bit for bit."""
    rows, pose, o = case
    axis, offsets = _axis(pose), np.linspace(-0.5 * mm, 0.5 * mm, 9)
    freqs = np.vstack([FREQS5, [[2e4, 2e4], [-4e4, 3e3]]])
    st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
    got = abi.psf_geo_otf(rows, *pose, axis, offsets, freqs, centers=st[:, [fr.CX, fr.CZ]])
    _check_geo(rows, pose, axis, offsets, st[:, [fr.CX, fr.CZ]], freqs, got[:3], [0, 8], [0, 6])
    assert np.array_equal(_bits(got[2]), _bits(st[:, fr.S]))


@pytest.mark.parametrize("nf,M", [(1, 1), (255, 1), (257, 1), (51, 5), (1, 257)])
def test_geometric_point_blocks(case, nf, M):
    """n_freqs * M = 1, 255, 257: a partial block of pairs and a second one, by frequencies and by planes.  Four pairs against the exact
    values, and every pair bit for bit what a call for it alone returns on a sample of them (the order of a pair's sum does not depend on
    the pairs asked for along with it)."""
    rows, pose, o = case
    rows, axis = rows[:300], _axis(pose)
    offsets = np.linspace(-0.5 * mm, 0.5 * mm, M) if M > 1 else np.array([0.2 * mm])
    t = (np.arange(nf) + 0.5) / nf
    freqs = np.stack([4.5e4 * np.cos(7 * t) * (1 - 0.5 * t), 4.5e4 * np.sin(5 * t + 0.3)], axis=1)
    assert nf * M in (1, 255, 257) and (freqs != 0).all()
    mtf, otf, sums, _ = abi.psf_geo_otf(rows, *pose, axis, offsets, freqs)
    assert mtf.shape == (M, nf) and np.isfinite(mtf).all()
    planes, fsel = sorted({0, M - 1}), sorted({0, nf - 1})
    _check_geo(rows, pose, axis, offsets, None, freqs, (mtf, otf, sums), planes, fsel)
    for m in sorted({0, M // 2, M - 1}):
        for q in sorted({0, nf // 3, nf - 2 if nf > 1 else 0, nf - 1}):
            one = abi.psf_geo_otf(rows, *pose, axis, offsets[m:m + 1], freqs[q:q + 1])
            for a, b in zip(one[:3], (mtf[m, q:q + 1], otf[m, q:q + 1], sums[m:m + 1])):
                assert np.array_equal(_bits(a).ravel(), _bits(b).ravel()), (m, q)


@pytest.mark.parametrize("record", [True, False])
def test_geometric_subsets_and_resident_rows_bit_for_bit(record):
    """A subset of planes and frequencies equals the full call; resident rows equal host rows, after a solve with the segment log and
    after a detector-only one."""
    rows, pose, o, (eng, dev, res, bundle) = _solve(2100, record=record, keep=True)
    sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
    try:
        axis, offsets = _axis(pose), np.linspace(-0.5 * mm, 0.5 * mm, 11)
        st, _ = abi.psf_focus_stats(rows, *pose, axis, offsets)
        cen = st[:, [fr.CX, fr.CZ]]
        full = abi.psf_geo_otf(rows, *pose, axis, offsets, FREQS5, centers=cen)
        assert np.array_equal(_bits(full[2]), _bits(st[:, fr.S]))
        ps, fs = [9, 0, 4], [3, 1]
        part = abi.psf_geo_otf(rows, *pose, axis, offsets[ps], FREQS5[fs], centers=cen[ps])
        for a, b in zip(part[:3], (full[0][np.ix_(ps, fs)], full[1][np.ix_(ps, fs)], full[2][ps])):
            assert np.array_equal(_bits(a), _bits(b))
        ptr, cnt, d = sol._psf_resident_rows(0)
        assert cnt == 2100
        resident = abi.psf_geo_otf(None, *pose, axis, offsets, FREQS5, centers=cen, device=d, hits_device_ptr=ptr, n_hits=cnt)
        for a, b in zip(resident[:3], full[:3]):
            assert np.array_equal(_bits(a), _bits(b))
    finally:
        sol.handle = None  # the engine frees the result
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def test_geometric_row_parallel_to_the_planes_reads_nan(case):
    rows, pose, o = case
    flat = rows[:300].copy()
    flat[7, 3:6] = [1.0, 0.0, 0.0]
    frame = (pose[0], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))  # nrm = (0, -1, 0): row 7 runs in the plane
    mtf, otf, sums, _ = abi.psf_geo_otf(flat, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4], FREQS5[:2])
    assert np.isnan(mtf).all() and np.isnan(otf.real).all() and np.isnan(otf.imag).all() and np.isnan(sums).all()
    flat[7] = rows[7]
    mtf, otf, sums, _ = abi.psf_geo_otf(flat, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4], FREQS5[:2])
    assert np.isfinite(mtf).all() and np.isfinite(sums).all()


# ------------------------------------------------------------------------------------------------ diffraction
@pytest.mark.parametrize("n,M", [(5, 1), (17, 1), (5, MP + 1), (17, MP + 1)])
def test_diffraction_transform_of_the_stack(case, n, M):
    """The image equals bmo_psf_through_focus bit for bit; the transfer function against the exact transform of that image; sums is the
    transform at f = 0.  n = 5: one partial block of points; n = 17: a second one; M = MP + 1 crosses the chunk of the stack."""
    rows, pose, o = case
    rows = rows[:600]
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    pitch = max(np.abs(np.diff(xs)).max(), np.abs(np.diff(zs)).max())
    freqs = np.vstack([[[0.0, 0.0]], FREQS5 / np.abs(FREQS5).max() * 0.45 / pitch])  # up to 0.9 of what the pitch carries (checked below)
    bmo.components.mtf_check_pitch(xs, zs, freqs)
    mtf, otf, sums, I, ms = abi.psf_otf(rows, *pose, d, xs, zs, freqs, want_intensity=True)
    assert mtf.shape == otf.shape == (M, 6) and I.shape == (M, n, n) and ms > 0
    assert np.array_equal(_bits(I), _bits(abi.psf_through_focus(rows, *pose, d, xs, zs)[0]))
    assert np.array_equal(_bits(otf[:, 0].real), _bits(sums)) and not otf[:, 0].imag.any()
    for m in sorted({0, M - 1, M // 2}):
        T, total = mr.otf_exact(I[m], xs, zs, freqs)
        assert abs(sums[m] - total) <= fr.gamma(2 * n) * total
        for q in range(len(freqs)):
            bound = mr.otf_bound(total, xs, zs, freqs[q], abs(T[q]))
            err = max(abs(otf[m, q].real - T[q].real), abs(otf[m, q].imag - T[q].imag))
            want = abs(T[q]) / total
            assert err <= bound < 1e-12 * total, (m, q, err, bound)
            assert abs(mtf[m, q] - want) <= mr.mtf_bound(bound, total, want, 2 * n) + fr.U * want, (m, q)
        assert mtf[m, 0] == 1.0 and mtf[m, 1:].max() < 1.0
    none = abi.psf_otf(rows[:0], *pose, d, xs, zs, freqs, want_intensity=True)
    assert not none[1].any() and not none[2].any() and not none[3].any() and np.isnan(none[0]).all()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_detector_and_solution_read_the_same_mtf():
    """PSFDetector.mtf on the copied rows and EngineSolution.psf_mtf on the resident ones, both kinds, bit for bit; the window of the
    diffraction kind comes from mtf_window (wavefront statistics and the Zernike pupil) on both paths."""
    rows, pose, o, (eng, dev, res, bundle) = _solve(600, record=False, keep=True)
    sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
    psfd = bmo.PSFDetector(10 * mm)
    psfd.data, psfd.position, psfd.orientation = rows, (lambda: pose[0]), (lambda: o)
    offsets = [-0.2 * mm, 0.0, 0.2 * mm]
    freqs = bmo.components.mtf_frequencies(3e4, 7, 30.0)
    try:
        for kw in (dict(kind="geometric"), dict(kind="geometric", follow=None, axis=_axis(pose)), dict(kind="diffraction"),
                   dict(kind="diffraction", n=24, half_width=1.5e-4, follow=None)):
            got, want = sol.psf_mtf(0, pose[0], o, freqs, offsets=offsets, **kw), psfd.mtf(freqs, offsets=offsets, **kw)
            assert got[0].shape == (3, 7) and got[3].shape == (3, 12) and sol.readout_ms > 0
            for a, b in zip(got, want):
                assert np.array_equal(_bits(a), _bits(b)), kw
            assert np.isfinite(got[0]).all() and np.abs(got[0][:, 0] - 1.0).max() < 1e-12 and (got[0] <= 1 + 1e-12).all()
        st = got[3]
        geo = psfd.mtf(freqs, offsets=offsets, kind="geometric")
        direct = abi.psf_geo_otf(rows, *pose, o[:, 1], offsets, freqs, centers=st[:, [fr.CX, fr.CZ]])
        assert np.array_equal(_bits(geo[1]), _bits(direct[1]))
        with pytest.raises(ValueError, match="alias"):
            psfd.mtf([[0.0, 0.0], [1e6, 0.0]], n=8, half_width=1e-4)
        with pytest.raises(ValueError, match="alias"):
            sol.psf_mtf(0, pose[0], o, [[0.0, 1e6]], n=8, half_width=1e-4)
    finally:
        sol.handle = None  # the engine frees the result
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def test_resident_rows_are_refused_where_they_are_not_psf_rows():
    """EngineSolution.psf_mtf asks the library for the rows (bmo_result_psf_rows): a slot of another detector kind is BMO_ERR_INVALID, a
    GaussianBeamlet solution BMO_ERR_UNSUPPORTED."""
    import scenes

    psfd, spot = bmo.PSFDetector(5 * mm), bmo.Spotdetector(5 * mm)
    bmo.translate3d(psfd, [-5 * mm, 50 * mm, 0])
    bmo.translate3d(spot, [5 * mm, 50 * mm, 0])
    bundle = scenes.disc_bundle(64, center=[0, 0, 0], direction=[0, 1, 0], diameter=18 * mm, lam=1e-6, jitter=0.0)
    sc = bmo.CompiledScene(bmo.System([psfd, spot]), bundle.lambdas)
    _, sol = bmo.system._engine_solve(sc, bundle, 100, None)
    try:
        kinds = {type(dd): slot for slot, dd in enumerate(sc.detectors)}
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        out = sol.psf_mtf(kinds[bmo.PSFDetector], pos, ori, [[0.0, 0.0], [1e3, 0.0]], kind="geometric")
        assert out[0].shape == (1, 2) and out[0][0, 0] == 1.0
        for slot in (kinds[bmo.Spotdetector], -1, 2):
            for kind in ("geometric", "diffraction"):
                with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-1\)"):
                    sol.psf_mtf(slot, pos, ori, [[0.0, 0.0]], kind=kind, n=4, half_width=1e-4)
    finally:
        sol.free()
    system3, _ = scenes.c2_scene()
    b3 = scenes.c3_bundle(64)
    _, sol3 = bmo.system._engine_solve(bmo.CompiledScene(system3, b3.lambdas), b3, 100, None)
    try:
        with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-4\).*GaussianBeamlet"):
            sol3.psf_mtf(0, np.zeros(3), np.eye(3), [[0.0, 0.0]], kind="geometric")
    finally:
        sol3.free()
