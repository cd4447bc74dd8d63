"""The yardsticks of the OPD map tests, checked without a GPU: the numpy restatement of include/bmo.h "OPD map read-out" against the exact
per-bin means inside the derived bound of tests/opd_ref.py (satisfiable, not vacuous, and with teeth), the info enum, the exports, the
refusals that need no device, and the Python layer's `remove` mapping."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import opd_ref as od
import psf_stats_ref as pr
import zernike_ref as zr

INVALID, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def _host_info(rows, pose, pupil=None):
    """the doubles X_REF .. W_MEAN a call would return, evaluated sequentially on the host (the restatement takes them as data)"""
    x, z = pr.local_xz(rows, *pose)
    w = rows[:, 7]
    u, v = zr.cosines(rows, pose[1], pose[2])
    info = np.full(od.INFO_N, np.nan)
    s = float(np.cumsum(w)[-1])
    info[od.N], info[od.S] = len(rows), s
    info[od.X_REF], info[od.Z_REF] = np.cumsum(w * x)[-1] / s, np.cumsum(w * z)[-1] / s
    if pupil is None:
        info[od.U0], info[od.V0] = np.cumsum(w * u)[-1] / s, np.cumsum(w * v)[-1] / s
        info[od.RHO] = np.sqrt(((u - info[od.U0]) * (u - info[od.U0]) + (v - info[od.V0]) * (v - info[od.V0])).max())
    else:
        info[od.U0], info[od.V0], info[od.RHO] = pupil
    W = pr.paths(rows, pr.ref_point(*pose, info[od.X_REF], info[od.Z_REF]))
    info[od.W_MEAN] = np.cumsum(w * W)[-1] / s
    return info


@pytest.mark.parametrize("rows_n,n,pupil", [(300, 7, None), (300, 1, None), (5000, 64, None), (5000, 32, (0.0, 0.0, 0.03)), (65, 2, None)])
def test_restatement_is_inside_the_bound_of_the_exact_means(pose, rows_n, n, pupil):
    rows = pr.synthetic_rows(rows_n, 7 + rows_n, pose)
    info = _host_info(rows, pose, pupil)
    coef = np.array([1e-9, 3e-9, -2e-9])
    proj, E, x, y = od.rows_of(rows, pose, info, 1, coef)
    R = od.restate(proj, E, x, y, n)
    assert R[od.STATUS] == 0 and R[od.N_BAD] == 0
    assert int(R["count"].sum()) + R[od.N_OUTSIDE] == rows_n
    if pupil is None:
        assert R[od.N_OUTSIDE] == 0 and R[od.N_OUT] <= 1
    else:
        assert 0 < R[od.N_OUTSIDE] < rows_n and R[od.N_OUT] >= R[od.N_OUTSIDE]
    # |q_h| <= 2^(61 - b): no bin can leave int64
    b = (rows_n - 1).bit_length()
    assert np.abs(R["q"]).max() <= 2 ** (61 - b) and np.abs(R["p"]).max() <= 2 ** (61 - b) and np.abs(R["q"]).max() >= 2 ** (59 - b)
    bad, worst, ex = od.map_violations(R["opd"], R, proj, E, n)
    assert bad == [] and len(ex) == R[od.N_FILLED]
    big = np.nanmax(np.abs(R["opd"]))
    print("%d rows, n = %d: %d bins filled, SH_Q %d SH_P %d, max |opd| %.3g m, largest bound %.3g m" % (rows_n, n, len(ex), R[od.SH_Q], R[od.SH_P], big, float(worst)))
    if rows_n == 5000:  # non-vacuity
        assert float(worst) < 1e-6 * big
    assert np.array_equal(R["weight"] > 0, R["count"] > 0)
    assert R[od.MAP_LO] == np.nanmin(R["opd"]) and R[od.MAP_HI] == np.nanmax(R["opd"])


def test_the_exact_equality_has_teeth(pose):
    """One row in the neighbouring bin, or one q_h off by one, changes the integers (and the first the counts)."""
    rows = pr.synthetic_rows(300, 11, pose)
    info = _host_info(rows, pose)
    proj, E, x, y = od.rows_of(rows, pose, info, 0, None)
    n = 7
    R = od.restate(proj, E, x, y, n)
    h = int(np.argmax((R["key"] >= 0) & (R["key"] % n < n - 1)))
    x2 = x.copy()
    x2[h] += 2.0 / n  # one bin along u
    R2 = od.restate(proj, E, x2, y, n)
    assert not np.array_equal(R2["count"], R["count"]) and not np.array_equal(R2["raw"], R["raw"])
    assert int(np.abs(R2["count"] - R["count"]).sum()) == 2
    raw3 = R["raw"].copy()
    raw3[R["key"][h], 0] += 1
    assert not np.array_equal(raw3, R["raw"])
    k = R["key"][h]  # (a sum above 2^53 may round to the same double: the integers are what the GPU tests compare)
    # a map moved by 1e-6 of its largest value leaves the bound
    moved = R["opd"].copy()
    moved[k] += 1e-6 * np.nanmax(np.abs(R["opd"]))
    bad, _, _ = od.map_violations(moved, R, proj, E, n)
    assert [v[0] for v in bad] == [k]


def test_status_2_keeps_the_counts(pose):
    rows = pr.synthetic_rows(64, 3, pose)
    info = _host_info(rows, pose)
    proj, E, x, y = od.rows_of(rows, pose, info, 0, None)
    want = od.restate(proj, E, x, y, 2)["count"]
    proj[5] = np.nan
    R = od.restate(proj, E, x, y, 2)
    assert R[od.STATUS] == 2 and R[od.N_BAD] == 1 and np.isnan(R["opd"]).all() and np.isnan(R["weight"]).all() and not R["raw"].any()
    assert np.array_equal(R["count"], want)


def test_shift_and_bins():
    assert od.shift(0.0, 5) == 0 and od.shift(1.0, 0) == 60 and od.shift(1.5, 3) == 57 and od.shift(0.75, 3) == 58
    assert od.shift(5e-324, 0) == 1000 and od.shift(1e308, 30) == 60 - 30 - 1023 and od.shift(1e308, 40) == -1000
    inside, key = od.bins([-1.0, 1.0, 0.0, np.nan, 1.0000000000000002, -0.0, np.nextafter(0.0, -1)], [-1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 4)
    assert inside.tolist() == [True, True, True, False, False, True, True]
    assert key.tolist() == [0, 15, 10, -1, -1, 14, 10]  # -5e-324 + 1.0 rounds to 1.0: the bin of 0


# ------------------------------------------------------------------------------------------------ the header, exports, refusals
def test_header_enum_equals_the_abi_columns():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmo.h")).read(), flags=re.S)
    body = re.search(r"enum bmo_opd_info \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(",") if item.strip())}
    assert len(enum) == 20 and sorted(enum.values()) == list(range(20))
    assert int(re.search(r"#define BMO_OPD_INFO_N (\d+)", hdr).group(1)) == 20 == abi.OPD_INFO_N == od.INFO_N
    assert int(re.search(r"#define BMO_OPD_MAX_N (\d+)", hdr).group(1)) == 4096 == abi.OPD_MAX_N == od.MAX_N
    for name, i in enum.items():
        short = name[len("BMO_OPD_"):]
        short = "N" if short == "N_ROWS" else short
        assert getattr(abi, "OPD_" + short) == i and getattr(od, short) == i, name
    zern = re.search(r"enum bmo_zernike_info \{(.*?)\};", hdr, flags=re.S).group(1)
    zern = {k.strip(): int(v) for k, v in (item.split("=") for item in zern.split(",") if item.strip())}
    for name in ("N_ROWS", "STATUS", "S", "X_REF", "Z_REF", "U0", "V0", "RHO", "W_MEAN", "E_LO", "E_HI", "N_OUT"):
        assert enum["BMO_OPD_" + name] == zern["BMO_ZERNIKE_" + name], name
    assert enum["BMO_OPD_E_RMS"] == zern["BMO_ZERNIKE_FIT_RMS"]
    src = open(os.path.join(ROOT, "beamletoptics.jl_amd", "csrc", "bmo_readout.inc.hpp")).read()
    assert int(re.search(r"constexpr int OPD_LDS_BINS = (\d+);", src).group(1)) == od.LDS_BINS


def _lib():
    return abi.load_engine()


def test_library_exports_both_entries():
    lib = _lib()
    for name in ("bmo_psf_opd_map", "bmo_psf_opd_map_sweep"):
        assert getattr(lib, name) is not None


def _opd_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, ref=None, pupil=None, order=1, coef=(0.0, 1e-9, 0.0), n=4, opd=True, weight=True, count=True,
            raw=False, info=True):
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    r = None if ref is None else np.array(ref, dtype=np.float64)
    q = None if pupil is None else np.array(pupil, dtype=np.float64)
    cf = None if coef is None else np.array(coef, dtype=np.float64)
    nb = min(max(n, 1), 64) ** 2
    a_opd, a_w, a_cnt, a_raw, a_info = np.full(nb, 7.0), np.full(nb, 7.0), np.full(nb, 7, dtype=np.int64), np.full(2 * nb, 7, dtype=np.int64), np.full(20, 7.0)
    ptr = lambda a, on: a.ctypes.data_as(dp) if on else None  # noqa: E731
    rc = _lib().bmo_psf_opd_map(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2),
                                None if r is None else r.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), order,
                                None if cf is None else cf.ctypes.data_as(dp), n, 0, ptr(a_opd, opd), ptr(a_w, weight), a_cnt.ctypes.data_as(ip) if count else None,
                                a_raw.ctypes.data_as(ip) if raw else None, ptr(a_info, info), None)
    if rc != 0:  # a refused call writes nothing
        assert (a_opd == 7).all() and (a_w == 7).all() and (a_cnt == 7).all() and (a_raw == 7).all() and (a_info == 7).all()
    return rc


def test_refusals_without_a_device():
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(opd=False), dict(weight=False), dict(count=False),
               dict(info=False), dict(order=-1, coef=None), dict(order=7), dict(n=0), dict(n=-3), dict(n=4097), dict(order=1, coef=None), dict(order=2, coef=None),
               dict(coef=(0.0, math.nan, 0.0)), dict(coef=(math.inf, 0.0, 0.0)), dict(order=0, coef=(math.nan,)), dict(pupil=(0.0, 0.0, 0.0)),
               dict(pupil=(0.0, 0.0, -0.03)), dict(pupil=(0.0, 0.0, math.inf)), dict(pupil=(math.nan, 0.0, 0.03)), dict(pupil=(0.0, math.inf, 0.03))):
        assert _opd_rc(**kw) == INVALID, kw
        assert b"bmo_psf_opd_map" in _lib().bmo_last_error()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    o, m, cnt, nf = np.zeros(3), np.zeros(16), np.zeros(16, dtype=np.int64), np.zeros(20)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    assert _lib().bmo_psf_opd_map_sweep(None, 0, 1, p(o), p(o), p(o), None, None, 0, None, 4, p(m), p(m), cnt.ctypes.data_as(ip), None, p(nf), None) == INVALID
    assert b"bmo_psf_opd_map_sweep" in _lib().bmo_last_error()


def test_valid_arguments_need_a_device():
    """No CPU fallback: with valid arguments the call gets as far as looking for a device."""
    for kw in (dict(), dict(ref=(1e-4, 0.0)), dict(pupil=(0.0, 0.01, 0.04), raw=True), dict(hits=False, n_hits=0), dict(order=0, coef=None), dict(order=0, coef=(1e-9,)),
               dict(order=6, coef=tuple([1e-9] * 28)), dict(n=1), dict(n=64)):
        rc = _opd_rc(**kw)
        assert rc == (NO_DEVICE if _lib().bmo_device_count() == 0 else 0), (kw, _lib().bmo_last_error())


# ------------------------------------------------------------------------------------------------ the Python layer
def test_remove_maps_to_zernike_terms():
    cp = bmo.components
    t4 = cp.zernike_terms(4)
    assert cp.opd_remove_terms("none", 4) == []
    assert cp.opd_remove_terms("tilt", 4) == [(0, 0), (1, -1), (1, 1)] == [t for t in t4 if t[0] <= 1]
    assert cp.opd_remove_terms("defocus", 4) == [(0, 0), (1, -1), (1, 1), (2, 0)]
    assert cp.opd_remove_terms("fit", 4) == t4 and cp.opd_remove_terms("fit", 0) == [(0, 0)]
    assert cp.opd_remove_terms("defocus", 1) == [(0, 0), (1, -1), (1, 1)]  # no (2, 0) at order 1
    assert cp.opd_remove_terms([(4, 0), (0, 0)], 4) == [(0, 0), (4, 0)]
    for bad in ("piston", [(5, 1)], [(2, 1)]):
        with pytest.raises(ValueError):
            cp.opd_remove_terms(bad, 4)
    # the coefficients that reach the map: the fit's, zero at the terms that are kept, about the fit's reference point and pupil
    fit = np.arange(1.0, 16.0)
    zi = np.zeros(13)
    zi[[abi.ZERN_X_REF, abi.ZERN_Z_REF, abi.ZERN_U0, abi.ZERN_V0, abi.ZERN_RHO]] = (1e-4, -2e-4, 0.01, -0.02, 0.05)
    seen = {}

    def map_fn(order, cf, ref, pupil):
        seen.update(order=order, cf=cf, ref=ref, pupil=pupil)
        return np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2), dtype=np.int64), np.zeros(20)

    out = cp.psf_opd_map(lambda order, ref, pupil: (fit, zi), map_fn, n=2, order=4, remove="defocus")
    want = np.zeros(15)
    want[[0, 1, 2, 4]] = fit[[0, 1, 2, 4]]
    assert len(out) == 5 and np.array_equal(out[4], want) and np.array_equal(seen["cf"], want) and seen["order"] == 4
    assert tuple(seen["ref"]) == (1e-4, -2e-4) and tuple(seen["pupil"]) == (0.01, -0.02, 0.05)
    out = cp.psf_opd_map(None, map_fn, n=2, order=4, remove="none", ref=(1.0, 2.0))
    assert seen["order"] == 0 and seen["cf"] is None and seen["ref"] == (1.0, 2.0) and seen["pupil"] is None and out[4].shape == (1,)
    us, vs = cp.opd_axes(np.array([0, 0, 0, 0, 0, 0.01, -0.02, 0.05] + [0] * 12, dtype=np.float64), 4)
    assert np.allclose(us, 0.01 + 0.05 * np.array([-0.75, -0.25, 0.25, 0.75])) and np.allclose(vs, -0.02 + 0.05 * np.array([-0.75, -0.25, 0.25, 0.75]))
