"""The polychromatic read-out without a GPU: the numpy statement of the band split, the coefficient and combination rules by hand-computed
values, the chromatic focus on synthetic statistics, and the argument checks the library makes before it looks for a device."""
import os
import re

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import poly_ref as po

cp = bmo.components
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_split_is_the_masked_rows_in_order():
    ks = [3.0, 1.0, 2.0, 9.0]  # the caller's order; 9.0 has no row
    band = np.array([0, 1, 1, 2, 0, 4, 5, 1, 0, 2])  # 4: an unlisted key, 5: NaN
    rows = po.synthetic_rows(band, ks + [7.0, np.nan])
    got, unmatched = po.band_split(rows, ks)
    assert [len(g) for g in got] == [3, 3, 2, 0] and unmatched == 2
    assert np.array_equal(got[0], rows[[0, 4, 8]]) and np.array_equal(got[1], rows[[1, 2, 7]]) and np.array_equal(got[2], rows[[3, 9]])
    dk, dc, dn = po.discover(rows)
    assert dk.tolist() == [1.0, 2.0, 3.0, 7.0] and dc.tolist() == [3, 2, 3, 1] and dn == 1
    # -0 == +0: one band by the compare, whatever the sign bit
    z = po.synthetic_rows([0, 1, 0], [0.0, -0.0])
    assert len(po.band_split(z, [0.0])[0][0]) == 3 and len(po.discover(z)[0]) == 1


def test_poly_coefficients_by_hand():
    S = [2.0, 4.0, 0.5]
    assert cp.poly_coefficients(None, S).tolist() == [0.25, 0.0625, 4.0]
    assert cp.poly_coefficients([1.0, 2.0, 0.5], S).tolist() == [0.25, 0.125, 2.0]
    assert cp.poly_coefficients([1.0, 2.0, 0.5], S, normalize=None).tolist() == [1.0, 2.0, 0.5]
    assert cp.poly_coefficients(None, S, normalize=None).tolist() == [1.0, 1.0, 1.0]
    assert cp.poly_coefficients([3.0, 5.0], [2.0, np.nan]).tolist() == [0.75, 0.0]  # a band without rows has no statistics: coefficient 0
    assert cp.poly_coefficients([3.0, 5.0], [0.0, 2.0]).tolist() == [0.0, 1.25]
    assert cp.poly_coefficients([3.0], [3.0])[0] == 3.0 / (3.0 * 3.0)  # w / (S * S), not (w / S) / S
    for bad in (dict(weights=[1.0], S=S), dict(weights=[1.0, np.inf, 1.0], S=S), dict(weights=None, S=S, normalize="peak")):
        with pytest.raises(ValueError):
            cp.poly_coefficients(**bad)


def test_the_combination_runs_left_to_right():
    """((c0 I0 + c1 I1) + c2 I2): with I = (2^53, 1, -2^53) the first add absorbs the 1 and the sum is 0; right to left it would be 1."""
    big = 2.0 ** 53
    images = np.array([[big, 1.0], [1.0, 2.0], [-big, 3.0]])
    assert cp.poly_combine([1.0, 1.0, 1.0], images).tolist() == [0.0, 6.0]
    assert (images[0] + (images[1] + images[2])).tolist() == [1.0, 6.0]  # the other association differs: the order is observable
    # a multiply and an add, not a fused multiply-add: 0.1 * 3 rounds to 0.30000000000000004 before the add
    assert cp.poly_combine([1.0, 0.1], [[-0.3], [3.0]])[0] == (0.1 * 3.0) + -0.3 == 5.551115123125783e-17
    c, I = [0.25, -1.5, 3.0], np.random.Generator(np.random.PCG64(3)).standard_normal((3, 4, 5))
    assert np.array_equal(po.bits(cp.poly_combine(c, I)), po.bits(po.combine(c, I)))
    assert np.array_equal(po.bits(cp.poly_combine(c, I)), po.bits((c[0] * I[0] + c[1] * I[1]) + c[2] * I[2]))
    with pytest.raises(ValueError):
        cp.poly_combine([], [])


def _synthetic_stats(offsets, focus, slope, cx, drift):
    """Focus statistics of a band that focuses at `focus`: RMS_R = hypot(1e-6, slope (t - focus)), CX = cx + drift t, CZ = -CX / 2."""
    st = np.zeros((len(offsets), abi.FOCUS_STAT_N))
    st[:, abi.FOCUS_N], st[:, abi.FOCUS_S] = 100, 100.0
    st[:, abi.FOCUS_RMS_R] = np.hypot(1e-6, slope * (offsets - focus))
    st[:, abi.FOCUS_CX] = cx + drift * offsets
    st[:, abi.FOCUS_CZ] = -st[:, abi.FOCUS_CX] / 2
    return st


def test_chromatic_focus_on_synthetic_statistics():
    off = np.linspace(-2e-3, 2e-3, 41)  # steps of 0.1 mm
    foci, cxs = [-0.8e-3, 0.33e-3, 1.0e-3], [1e-6, 2e-6, 4e-6]
    tables = [_synthetic_stats(off, f, 0.03, c, 1e-3) for f, c in zip(foci, cxs)]
    tables.append(np.full((41, abi.FOCUS_STAT_N), np.nan))  # a band without rows
    tables[3][:, abi.FOCUS_N] = 0
    asked = []

    def per_band(b, axis, offsets):
        asked.append((b, tuple(axis)))
        assert np.array_equal(offsets, off)
        return tables[b]

    st, focus, rms, cen, plane = cp.psf_chromatic_focus(per_band, [4.0, 3.0, 2.0, 1.0], off, (0.0, 1.0, 0.0))
    assert st.shape == (4, 41, 12) and asked == [(b, (0.0, 1.0, 0.0)) for b in range(4)]
    assert np.abs(focus[:3] - foci).max() < 0.05e-3 and np.isnan(focus[3]) and np.isnan(rms[3])  # inside half a step of the samples
    assert focus[0] < focus[1] < focus[2] and (rms[:3] <= 1e-6 * (1 + 1e-12) + 0.03 * 0.05e-3).all()
    want_plane = int(np.argmin(np.abs(off - np.mean(focus[:3]))))
    assert plane == want_plane and np.array_equal(cen[:3, 0], [c + 1e-3 * off[plane] for c in cxs]) and np.array_equal(cen[:3, 1], -cen[:3, 0] / 2)
    assert np.isnan(cen[3]).all()
    _, _, _, cen7, plane7 = cp.psf_chromatic_focus(per_band, [4.0, 3.0, 2.0, 1.0], off, (0.0, 1.0, 0.0), plane=7)
    assert plane7 == 7 and cen7[1, 0] == cxs[1] + 1e-3 * off[7]
    with pytest.raises(ValueError):
        cp.psf_chromatic_focus(per_band, [1.0], off, (0.0, 1.0, 0.0), plane=41)
    with pytest.raises(ValueError):
        cp.psf_chromatic_focus(per_band, [1.0], [], (0.0, 1.0, 0.0))


def test_the_library_refuses_bad_bands_before_it_looks_for_a_device():
    rows = po.synthetic_rows([0, 1, 0, 1], [1.0, 2.0])
    for ks in ([1.0, 1.0], [1.0, 2.0, 1.0], [0.0, -0.0], [1.0, np.nan], [np.inf], [-np.inf, 1.0], []):
        with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-1\)"):
            abi.psf_bands(rows, ks=ks)
    with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-6\)"):
        abi.psf_bands(rows, ks=np.arange(1.0, 66.0))
    with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-1\)"):
        abi.psf_bands(rows, ks=[1.0] * 65)  # equal keys are refused before the count
    with pytest.raises(RuntimeError, match=r"bmo_psf_bands_create failed \(-1\)"):
        abi.psf_bands(None, hits_device_ptr=0, n_hits=-1)
    lib = abi.load_engine()
    assert lib.bmo_psf_bands_info(None, None, None, None, None) == -1 and lib.bmo_psf_bands_get(None, 0, None, None, None) == -1
    assert lib.bmo_psf_bands_free(None) == 0
    assert lib.bmo_psf_poly_through_focus(None, None, None, None, None, 1, None, None, 1, None, None, None, None) == -1
    assert lib.bmo_psf_poly_otf(None, None, None, None, None, 1, None, None, 1, None, None, 1, None, None, None, None, None) == -1


def test_the_wrappers_check_their_arguments():
    e = np.eye(3)
    for fn, tail in ((abi.psf_poly_through_focus, ()), (abi.psf_poly_otf, ([[0.0, 0.0]],))):
        with pytest.raises(ValueError, match="PsfBands"):
            fn(None, e[0], e[0], e[2], [[0, 0, 0]], [0.0], [0.0], [1.0], *tail)
    assert abi.PSF_MAX_BANDS == int(re.search(r"#define BMO_PSF_MAX_BANDS (\d+)", open(os.path.join(ROOT, "include", "bmo.h")).read()).group(1))
    for name in ("bands", "chromatic_focus", "poly_through_focus", "poly_mtf"):
        assert callable(getattr(bmo.PSFDetector, name))
    for name in ("psf_bands", "psf_chromatic_focus", "psf_poly_through_focus", "psf_poly_mtf"):
        assert callable(getattr(bmo.system.EngineSolution, name))
