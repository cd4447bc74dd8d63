"""The yardsticks of the wavefront read-out tests, checked without a GPU: the derived bounds against a plain sequential evaluation
(satisfiable) and the one-pass variance (they have teeth), the conventions, the window rule of psf_axes_from_stats, the exports, the
refusals that need no device, and the Julia constants."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import psf_stats_ref as pr

INVALID, NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def test_the_pose_has_no_zero_component(pose):
    assert all(np.all(np.abs(v) > 1e-3) for v in pose[1:])


@pytest.mark.parametrize("n", [1, 2, 257, 4000])
def test_sequential_evaluation_is_inside_every_bound(pose, n):
    rows = pr.synthetic_rows(n, 3 + n, pose, two_wavelengths=(n == 257))
    for ref in (None, (pr.F_LOCAL[0] + 2e-7, pr.F_LOCAL[1] - 1e-7)):
        got = pr.two_pass_sequential(rows, *pose, ref=ref)
        assert pr.stat_violations(got, rows, *pose, ref=ref) == [], (n, ref)


def test_bounds_catch_the_one_pass_variance():
    rows, pose = pr.offset_wavefront()
    ref = pr.F_LOCAL
    got = pr.two_pass_sequential(rows, *pose, ref=ref)
    assert pr.stat_violations(got, rows, *pose, ref=ref) == []
    assert 5e-9 < got[pr.W_RMS] < 2e-8  # N(0, 10 nm) on 0.2 m
    bad = got.copy()
    bad[pr.W_RMS] = pr.one_pass_w_rms(rows, *pose, *ref)
    assert [v[0] for v in pr.stat_violations(bad, rows, *pose, ref=ref)] == ["W_RMS"]
    # the bound is tight enough to matter: far below the statistic itself
    x, z = pr.local_xz(rows, *pose)
    W = pr.paths(rows, pr.ref_point(*pose, *ref))
    assert float(pr.sum_bounds(pr.exact_stats(x, z, W, rows[:, 7]))[5]) < 1e-6 * got[pr.W_RMS]


def test_empty_and_single_row_conventions(pose):
    empty = np.full(pr.STAT_N, np.nan)
    empty[pr.N] = 0
    none = np.zeros((0, 9))
    assert pr.stat_violations(empty, none, *pose) == []
    assert pr.stat_violations(np.zeros(pr.STAT_N), none, *pose) != []
    assert pr.stat_violations(pr.two_pass_sequential(none, *pose), none, *pose) == []
    row = pr.synthetic_rows(1, 9, pose)
    one = pr.two_pass_sequential(row, *pose, ref=pr.F_LOCAL)
    assert one[pr.N] == 1 and one[pr.S] == row[0, 7] and one[pr.X_MIN] == one[pr.X_MAX] and one[pr.K_MIN] == one[pr.K_MAX]
    assert one[pr.W_LO] == one[pr.W_HI] and abs(one[pr.STREHL] - 1) < 1e-15
    assert bmo.components.psf_marechal(empty) != bmo.components.psf_marechal(empty)  # NaN


def test_focus_rows_are_a_perfect_focus_within_the_row_error(pose):
    rows, f = pr.focus_rows(300, 4, pose)
    W = pr.paths(rows, f)
    assert np.abs(W - pr.FOCUS_R).max() <= pr.focus_row_error(f)
    assert pr.focus_row_error(f) < 1e-15


# ------------------------------------------------------------------------------------------------ the window rule
def _hand_stats(K):
    rng = np.random.default_rng(8)
    st = np.zeros((K, abi.PSF_STAT_N))
    st[:, abi.PSF_N] = 10
    st[:, abi.PSF_CX], st[:, abi.PSF_CZ] = 1e-4 * rng.standard_normal(K), 1e-4 * rng.standard_normal(K)
    st[:, abi.PSF_X_MIN], st[:, abi.PSF_X_MAX] = st[:, abi.PSF_CX] - 3e-5 * rng.uniform(1, 2, K), st[:, abi.PSF_CX] + 3e-5 * rng.uniform(1, 2, K)
    st[:, abi.PSF_Z_MIN], st[:, abi.PSF_Z_MAX] = st[:, abi.PSF_CZ] - 2e-5 * rng.uniform(1, 2, K), st[:, abi.PSF_CZ] + 2e-5 * rng.uniform(1, 2, K)
    st[:, abi.PSF_HWX] = np.maximum(st[:, abi.PSF_CX] - st[:, abi.PSF_X_MIN], st[:, abi.PSF_X_MAX] - st[:, abi.PSF_CX])
    st[:, abi.PSF_HWZ] = np.maximum(st[:, abi.PSF_CZ] - st[:, abi.PSF_Z_MIN], st[:, abi.PSF_Z_MAX] - st[:, abi.PSF_CZ])
    return st


def test_axes_from_stats_restate_the_rule_of_psf_sample_axes():
    K, n = 5, 17
    st = _hand_stats(K)
    lr = bmo.linalg.linrange
    for kw in (dict(), dict(crop_factor=2.5), dict(center="bbox", crop_factor=3), dict(x_min=-1e-4, x_max=2e-4), dict(z_min=-3e-4, z_max=1e-4, x0_shift=1e-6),
               dict(x_min=-1e-4), dict(center="bbox", z0_shift=-2e-6)):
        xs, zs = bmo.components.psf_axes_from_stats(st, n=n, **kw)
        assert xs.shape == (K, n) and zs.shape == (K, n)
        crop = kw.get("crop_factor", 1.0)
        for c in range(K):
            s = st[c]
            if kw.get("center", "centroid") == "centroid":
                x0, z0, hx, hz = s[abi.PSF_CX], s[abi.PSF_CZ], s[abi.PSF_HWX], s[abi.PSF_HWZ]
            else:
                x0, z0 = (s[abi.PSF_X_MIN] + s[abi.PSF_X_MAX]) / 2, (s[abi.PSF_Z_MIN] + s[abi.PSF_Z_MAX]) / 2
                hx = max(abs(s[abi.PSF_X_MIN] - x0), abs(s[abi.PSF_X_MAX] - x0))
                hz = max(abs(s[abi.PSF_Z_MIN] - z0), abs(s[abi.PSF_Z_MAX] - z0))
            lim = [x0 - hx * crop, x0 + hx * crop, z0 - hz * crop, z0 + hz * crop]
            if "x_min" in kw and "x_max" in kw:
                lim[0:2] = kw["x_min"], kw["x_max"]
            if "z_min" in kw and "z_max" in kw:
                lim[2:4] = kw["z_min"], kw["z_max"]
            assert np.array_equal(xs[c], lr(lim[0], lim[1], n) + kw.get("x0_shift", 0.0)), (kw, c)
            assert np.array_equal(zs[c], lr(lim[2], lim[3], n) + kw.get("z0_shift", 0.0)), (kw, c)
            x1, z1 = bmo.components.psf_axes_from_stats(s, n=n, **kw)
            assert x1.shape == (n,) and np.array_equal(x1, xs[c]) and np.array_equal(z1, zs[c])


def test_axes_from_stats_agree_with_psf_sample_axes_on_rows(pose):
    """Statistics made from rows by the sequential evaluation: the bounding-box window is psf_sample_axes' bit for bit (extrema are exact),
    the centroid window when the statistics carry numpy's own centroid."""
    rows = pr.synthetic_rows(300, 2, pose)
    ori = np.zeros((3, 3))
    ori[:, 0], ori[:, 2] = pose[1], pose[2]
    st = pr.two_pass_sequential(rows, *pose)
    loc = bmo.components.psf_local_pos(rows, pose[0], ori)
    # psf_local_pos is a matrix product: its x_h may differ from the header's expression in the last bit, so restate the statistics on its values
    st[[pr.X_MIN, pr.X_MAX, pr.Z_MIN, pr.Z_MAX]] = loc[:, 0].min(), loc[:, 0].max(), loc[:, 1].min(), loc[:, 1].max()
    w = rows[:, 7]
    st[pr.CX], st[pr.CZ] = (w * loc[:, 0]).sum() / w.sum(), (w * loc[:, 1]).sum() / w.sum()
    st[pr.HWX], st[pr.HWZ] = np.abs(loc[:, 0] - st[pr.CX]).max(), np.abs(loc[:, 1] - st[pr.CZ]).max()
    for kw in (dict(center="bbox", crop_factor=5), dict(crop_factor=2), dict(x0_shift=1e-6)):
        want = bmo.components.psf_sample_axes(rows, pose[0], ori, n=33, **kw)
        got = bmo.components.psf_axes_from_stats(st, n=33, **kw)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), kw


def test_marechal():
    st = np.zeros((3, abi.PSF_STAT_N))
    k = 2 * math.pi / 1e-6
    st[:, abi.PSF_K_MIN] = k
    st[:, abi.PSF_K_MAX] = [k, k, 1.25 * k]
    st[:, abi.PSF_W_RMS] = [0.0, 1e-6 / 14, 1e-8]
    m = bmo.components.psf_marechal(st)
    assert m[0] == 1.0 and abs(m[1] - math.exp(-(2 * math.pi / 14) ** 2)) < 1e-15 and math.isnan(m[2])
    assert bmo.components.psf_marechal(st[1]) == m[1]


# ------------------------------------------------------------------------------------------------ exports and refusals that need no device
def _lib():
    return abi.load_engine()


def test_library_exports_both_entries():
    lib = _lib()
    for name in ("bmo_psf_stats", "bmo_psf_stats_sweep"):
        assert getattr(lib, name) is not None
    assert abi.PSF_STAT_N == 21 and abi.PSF_K_MAX == 20


def _stats_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, ref=None, stats=True):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    r = None if ref is None else np.array(ref, dtype=np.float64)
    st = np.zeros(21)
    ptr = lambda a, on: a.ctypes.data_as(dp) if on else None  # noqa: E731
    return _lib().bmo_psf_stats(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2),
                                None if r is None else r.ctypes.data_as(dp), 0, ptr(st, stats), None)


def test_refusals_without_a_device():
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(stats=False)):
        assert _stats_rc(**kw) == INVALID, kw
        assert b"bmo_psf_stats" in _lib().bmo_last_error()
    dp = C.POINTER(C.c_double)
    o, st = np.zeros(3), np.zeros(21)
    assert _lib().bmo_psf_stats_sweep(None, 0, 1, o.ctypes.data_as(dp), o.ctypes.data_as(dp), o.ctypes.data_as(dp), None, st.ctypes.data_as(dp), None) == INVALID
    assert b"bmo_psf_stats_sweep" in _lib().bmo_last_error()


def test_valid_arguments_need_a_device():
    """No CPU fallback: with valid arguments the call gets as far as looking for a device (a null hits pointer is valid with n_hits = 0)."""
    for kw in (dict(), dict(ref=(1e-4, 0.0)), dict(hits=False, n_hits=0)):
        rc = _stats_rc(**kw)
        assert rc == (NO_DEVICE if _lib().bmo_device_count() == 0 else 0), (kw, _lib().bmo_last_error())


# ------------------------------------------------------------------------------------------------ the Julia binding
def test_julia_constants_equal_the_enum():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bmo.h")).read(), flags=re.S)
    body = re.search(r"enum bmo_psf_stat \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(",") if item.strip())}
    assert len(enum) == 21 and sorted(enum.values()) == list(range(21))
    assert int(re.search(r"#define BMO_PSF_STAT_N (\d+)", hdr).group(1)) == 21 == abi.PSF_STAT_N
    jl = open(os.path.join(root, "julia", "GPUSystem.jl")).read()
    m = re.search(r"^const (PSF_STAT_N_ROWS[A-Z_, ]+?) = Int32\.\((\d+):(\d+)\)$", jl, flags=re.M)
    names = [n.strip() for n in m.group(1).split(",")]
    assert (int(m.group(2)), int(m.group(3))) == (0, 20) and len(names) == 21
    for i, name in enumerate(names):
        assert enum["BMO_" + name] == i, name
        assert getattr(pr, name[len("PSF_STAT_"):] if name != "PSF_STAT_N_ROWS" else "N") == i, name
    assert re.search(r"^const PSF_STAT_N = Int32\(21\)$", jl, flags=re.M)
    for sym in ("bmo_psf_stats", "bmo_psf_stats_sweep"):
        assert "ccall((:%s, LIBBMO)" % sym in jl
    # the Python constants follow the same order
    for i, name in enumerate(names):
        assert getattr(abi, "PSF_" + (name[len("PSF_STAT_"):] if name != "PSF_STAT_N_ROWS" else "N")) == i
