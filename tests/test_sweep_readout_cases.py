"""include/bmo_sweep_readout.h is held to the rules include/bmo.h is held to (tests/test_state_cases.py): every entry it declares is
exported by the built library, has a ctypes signature of the same arity and a wrapper in bmo_amd.abi, and is reached by a case of
tests/sweep_readout_cases.py; bmo.h includes the header.  And the host planning that components.psf_through_focus / psf_mtf share with the
sweep path (focus_planes, through_focus_plan, mtf_geo_centers, mtf_image_grid) gives exactly what those two hand to their callbacks.
No device: the cases are not run here."""
import os
import re

import numpy as np
import pytest

import sweep_readout_cases as sw
from bmo_amd import abi
from bmo_amd import components as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bmo_psf_focus_stats_sweep", "bmo_psf_through_focus_sweep", "bmo_psf_geo_otf_sweep", "bmo_psf_otf_sweep")


def test_the_header_declares_the_four_entries_and_bmo_h_includes_it():
    assert set(sw.header_declarations()) == set(ENTRIES)
    text = open(os.path.join(ROOT, "include", "bmo.h"), encoding="utf-8").read()
    assert re.search(r'^#include "bmo_sweep_readout\.h"\s*$', text, re.M)
    assert "#define BMO_ABI_VERSION 1" in text or re.search(r"BMO_ABI_VERSION\s+1\b", text)


def test_every_entry_is_exported_with_a_signature_of_its_arity_and_a_wrapper():
    lib = abi.load_engine()
    for name, n_params in sw.header_declarations().items():
        fn = getattr(lib, name)  # AttributeError: the built library does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, (name, n_params)
        assert callable(getattr(abi, name[len("bmo_"):])), name


def test_every_entry_has_a_case():
    declared = set(sw.header_declarations())
    covered = set().union(*(f.entries for f in sw.CASES))
    assert covered == declared, (sorted(declared - covered), sorted(covered - declared))
    names = [f.name for f in sw.CASES]
    assert len(names) == len(set(names)) and all(f.group == sw.GROUP for f in sw.CASES)


# ------------------------------------------------------------------------------------------------ the shared planning
def _stats(M, seed, nan_plane=None):
    """synthetic focus statistics [M, 12] of a bundle that comes to a focus near the middle plane"""
    rng = np.random.default_rng(seed)
    st = np.zeros((M, abi.FOCUS_STAT_N))
    st[:, abi.FOCUS_N] = 500
    st[:, abi.FOCUS_S] = 321.5
    st[:, abi.FOCUS_CX], st[:, abi.FOCUS_CZ] = 1e-5 * rng.uniform(-1, 1, M), 1e-5 * rng.uniform(-1, 1, M)
    st[:, abi.FOCUS_RMS_R] = 1e-6 + 1e-5 * np.abs(np.arange(M) - M // 2 + 0.3)
    st[:, abi.FOCUS_HWX], st[:, abi.FOCUS_HWZ] = 3 * st[:, abi.FOCUS_RMS_R], 2.5 * st[:, abi.FOCUS_RMS_R]
    if nan_plane is not None:
        st[nan_plane, 1:] = np.nan
    return st


def _orientation():
    a, b = np.radians(7), np.radians(0.4)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return ry @ rx


@pytest.mark.parametrize("kw", [dict(), dict(follow=None), dict(window_plane=1, crop_factor=3.0), dict(half_width=2e-5), dict(half_width=(2e-5, 3e-5), follow=None),
                                dict(axis=[0.1, 0.9, -0.2])])
def test_through_focus_plan_is_what_psf_through_focus_hands_its_callbacks(kw):
    o, offsets = _orientation(), np.linspace(-1e-3, 1e-3, 7)
    st = _stats(7, 1, nan_plane=5)
    seen = {}

    def stats_fn(ax, off):
        seen["planes"] = (ax.copy(), off.copy())
        return st

    def stack_fn(d, xs, zs):
        seen["stack"] = (d.copy(), xs.copy(), zs.copy())
        return "I"

    xs, zs, d, I, st_out = cp.psf_through_focus(stats_fn, stack_fn, o, offsets, n=9, **kw)
    ax, off = cp.focus_planes(o, offsets, kw.get("axis"), kw.get("follow", "centroid"), "through_focus")
    assert np.array_equal(ax, seen["planes"][0]) and np.array_equal(off, seen["planes"][1])
    plan_kw = {k: v for k, v in kw.items() if k != "axis"}
    pxs, pzs, pd = cp.through_focus_plan(st, o, ax, off, n=9, **plan_kw)
    for got, want in ((pd, seen["stack"][0]), (pxs, seen["stack"][1]), (pzs, seen["stack"][2]), (pxs, xs), (pzs, zs), (pd, d)):
        assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert I == "I" and st_out is st and len(pxs) == 9 and pd.shape == (7, 3)


def test_the_plan_refuses_what_psf_through_focus_refuses():
    o = _orientation()
    empty = np.full((3, abi.FOCUS_STAT_N), np.nan)
    empty[:, abi.FOCUS_N] = 0
    with pytest.raises(ValueError, match="recorded no hit"):
        cp.through_focus_plan(empty, o, o[:, 1], np.zeros(3))
    flat = _stats(3, 2)
    flat[:, 1:] = np.nan
    with pytest.raises(ValueError, match="no plane has statistics"):
        cp.through_focus_plan(flat, o, o[:, 1], np.zeros(3))
    with pytest.raises(ValueError, match="no offsets"):
        cp.focus_planes(o, [], None, "centroid", "through_focus")
    with pytest.raises(ValueError, match="follow"):
        cp.focus_planes(o, [0.0], None, "chief", "mtf")
    for fn in (lambda: cp.psf_through_focus(lambda a, b: empty, None, o, np.zeros(3)), lambda: cp.psf_through_focus(lambda a, b: flat, None, o, np.zeros(3))):
        with pytest.raises(ValueError, match="through_focus"):
            fn()


@pytest.mark.parametrize("follow", ["centroid", None])
def test_mtf_planning_is_what_psf_mtf_hands_its_callbacks(follow):
    o, offsets = _orientation(), np.linspace(-1e-3, 1e-3, 5)
    st = _stats(5, 3, nan_plane=0)
    freqs = cp.mtf_frequencies(4e4, 6, azimuth_deg=30)
    window = (2 * np.pi / 1e-6, 0.0375, 1000)
    seen = {}

    def geo_fn(ax, off, fq, cen):
        seen["geo"] = (ax.copy(), off.copy(), fq.copy(), cen.copy())
        return "mtf", "otf", "sums"

    def otf_fn(d, xs, zs, fq):
        seen["otf"] = (d.copy(), xs.copy(), zs.copy())
        return "mtf", "otf", "sums"

    cp.psf_mtf(lambda ax, off: st, geo_fn, None, None, o, freqs, offsets=offsets, kind="geometric", follow=follow)
    cen = cp.mtf_geo_centers(st, follow)
    assert cen.shape == (5, 2) and np.array_equal(cen.view(np.uint64), seen["geo"][3].view(np.uint64))
    if follow is None:
        assert (cen == st[int(np.nanargmin(st[:, abi.FOCUS_RMS_R])), [abi.FOCUS_CX, abi.FOCUS_CZ]]).all()
    for kw in (dict(), dict(n=33), dict(half_width=3e-5), dict(half_width=3e-5, n=40)):
        cp.psf_mtf(lambda ax, off: st, None, otf_fn, lambda: window, o, freqs, offsets=offsets, kind="diffraction", follow=follow, **kw)
        hw, n = cp.mtf_image_grid(None if "half_width" in kw else window, freqs, **kw)
        assert n == kw.get("n", n) and (("half_width" in kw) == (hw == 3e-5))
        ax, off = cp.focus_planes(o, offsets, None, follow, "mtf")
        xs, zs, d = cp.through_focus_plan(st, o, ax, off, n=n, follow=follow, half_width=hw)
        for got, want in zip((d, xs, zs), seen["otf"]):
            assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), kw
        cp.mtf_check_pitch(xs, zs, freqs)
    assert cp.mtf_image_grid(window, freqs) == cp.mtf_window(*window, float(np.abs(freqs).max()))
