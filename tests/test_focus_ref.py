"""The yardsticks of the through-focus read-out tests, checked without a GPU: the 40-digit stack against the existing exact field, the
moved-detector identity in mpmath alone, the exact statistics of a fan whose crossing point is known, components.best_focus, and the
declarations, exports and refusals that need no device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import focus_ref as fr
import psf_stats_ref as pr
import readout_ref as rr

INVALID, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def test_exact_stack_at_zero_displacement_is_the_exact_field(pose):
    rows = pr.synthetic_rows(40, 3, pose)
    xs, zs = pr.F_LOCAL[0] + np.array([-2e-6, 0.0, 3e-6]), pr.F_LOCAL[1] + np.array([-1e-6, 2e-6])
    F = fr.through_focus_exact(rows, *pose, [[0.0, 0.0, 0.0]], xs, zs)
    assert F.shape == (1, 3, 2)
    assert np.array_equal(F[0], rr.psf_field_exact(rows, *pose, xs, zs))


def test_moved_detector_identity_in_mpmath(pose):
    """Rows on plane A propagated exactly to plane B = A moved by `shift` (hit' = hit + s dir, opl' = opl + s): the field of B's rows at B's
    point equals the through-focus plane of A's rows at the displacement `shift`, to 1e-30 relative.  This pins the sign of the factor and
    the frame of the displacement independently of the engine.  The identity needs unit directions (the phase moves by k s (1 - |dir|^2)),
    so the directions are normalised at 40 digits; with the doubles as they are, the two differ by that term and no more."""
    import mpmath as mp

    origin, e1, e2 = pose
    rows = pr.synthetic_rows(25, 5, pose)
    nrm = np.cross(e1, e2)
    for shift in (0.3e-3 * nrm, -0.2e-3 * nrm + 0.05e-3 * e1 - 0.02e-3 * e2):
        with mp.workdps(40):
            ex = lambda a: [mp.mpf(float(v)) for v in a]  # noqa: E731
            rows_a = [ex(r) for r in rows]
            for r in rows_a:
                nd = mp.sqrt(mp.fsum(v * v for v in r[3:6]))
                r[3:6] = [v / nd for v in r[3:6]]
            moved = fr.propagate_exact(rows_a, origin, e1, e2, shift)
            o, a1, a2, sh = ex(origin), ex(e1), ex(e2), ex(shift)
            for x, z in ((pr.F_LOCAL[0] + 4e-6, pr.F_LOCAL[1] - 3e-6), (1e-4, -2e-4)):
                p_b = [o[k] + sh[k] + mp.mpf(x) * a1[k] + mp.mpf(z) * a2[k] for k in range(3)]
                f_b = fr.field_exact_mp(moved, p_b)  # the moved detector's own rows at its own point
                f_a = fr.field_exact_mp(rows_a, p_b)  # plane A's rows at the displaced point: the through-focus plane
                assert abs(f_b - f_a) <= mp.mpf("1e-30") * abs(f_b), (shift, x, z)
                assert abs(f_b) > 0
            # the doubles as they are: the moved rows' field differs by at most k s | 1 - |dir|^2 | per unit of proj
            f_d = fr.field_exact_mp([ex(r) for r in rows], p_b)
            slack = max(float(r[8] * abs(m[6] - r[6]) * abs(1 - mp.fsum(mp.mpf(float(v)) ** 2 for v in d[3:6]))) for r, m, d in zip(rows_a, moved, rows))
            assert 0 < abs(f_d - f_a) <= slack * float(rows[:, 7].sum()) and slack < 1e-11
        # and through_focus_exact is that evaluation on the doubles
        F = fr.through_focus_exact(rows, origin, e1, e2, [shift], [1e-4], [-2e-4])[0, 0, 0]
        assert abs(F - complex(f_d)) <= 4 * fr.U * abs(F)
    # a wrong sign of the displacement is seen
    F_wrong = fr.through_focus_exact(rows, origin, e1, e2, [-shift], [1e-4], [-2e-4])[0, 0, 0]
    assert abs(F_wrong - F) > 1e-3 * abs(F)


def test_exact_statistics_of_a_three_ray_fan():
    """Three rays of equal weight recorded on the plane y = 0 at x = -a, 0, +a, aimed at the point (0, f, 0): at the offset t along y they
    stand at x = -a (1 - t / f), 0, a (1 - t / f): centroid 0, half-width a |1 - t / f|, RMS radius sqrt(2 / 3) of it, and all of them
    cross at t = f."""
    a, f = 0.25, 2.0  # binary fractions: the rows are exact
    rows = np.zeros((3, 9))
    for i, x0 in enumerate((-a, 0.0, a)):
        d = np.array([-x0, f, 0.0])
        rows[i, 0:3] = [x0, 0.0, 0.0]
        rows[i, 3:6] = d / np.linalg.norm(d)
        rows[i, 6:9] = [1.0, 0.5, 2 * math.pi / 1e-6]
    origin, e1, e2, axis = [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]  # e1 x e2 = -y: the sign of the normal cancels in s
    offsets = [0.0, 0.5, 2.0, 3.0]
    ex = fr.focus_stats_exact(rows, origin, e1, e2, axis, offsets)
    for t, e in zip(offsets, ex):
        w = a * abs(1 - t / f)
        assert e["n"] == 3 and e["s"] == 1.5
        for key, want in (("cx", 0.0), ("cz", 0.0), ("x_min", -w), ("x_max", w), ("z_min", 0.0), ("z_max", 0.0), ("hwx", w), ("hwz", 0.0),
                          ("rms_r", math.sqrt(2.0 / 3.0) * w), ("max_r", w)):
            assert abs(e[key] - want) <= 4 * fr.U * max(abs(want), a * 1e-3), (t, key, e[key], want)
    assert ex[2]["rms_r"] <= 1e-16  # the crossing point
    # the bounds are positive and of the size of a few u of the coordinates
    b = fr.stat_bounds(ex[1])
    assert all(b[k] > 0 for k in range(1, fr.STAT_N)) and b[fr.CX] < 1e-13 and b[fr.RMS_R] < 1e-13


def test_best_focus_on_a_sampled_parabola():
    x = np.array([-3.0, -1.0, 0.5, 2.0, 4.0])  # uneven spacing
    y = 2.0 * (x - 0.75) ** 2 + 1.5
    xv, yv = bmo.components.best_focus(x, y)
    assert abs(xv - 0.75) < 1e-14 and abs(yv - 1.5) < 1e-14
    xv, yv = bmo.components.best_focus(x, -y, kind="max")
    assert abs(xv - 0.75) < 1e-14 and abs(yv + 1.5) < 1e-14
    # at an end of the range: the end sample itself
    assert bmo.components.best_focus(x, (x + 10.0) ** 2) == (-3.0, 49.0)
    assert bmo.components.best_focus(x, (x - 10.0) ** 2) == (4.0, 36.0)
    assert bmo.components.best_focus(x, -(x - 10.0) ** 2, kind="max") == (4.0, -36.0)
    with pytest.raises(ValueError):
        bmo.components.best_focus(x, y, kind="least")
    with pytest.raises(ValueError):
        bmo.components.best_focus(x, y[:-1])


# ------------------------------------------------------------------------------------------------ declarations, exports, refusals
SYMBOLS = {"bmo_psf_through_focus": 15, "bmo_psf_focus_stats": 12}


def test_header_declares_both_entries():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmo.h")).read(), flags=re.S)
    for name, arity in SYMBOLS.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity, name
    body = re.search(r"enum bmo_focus_stat \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(",") if item.strip())}
    assert int(re.search(r"#define BMO_FOCUS_STAT_N (\d+)", hdr).group(1)) == len(enum) == abi.FOCUS_STAT_N == fr.STAT_N
    for name, col in enum.items():
        short = name[len("BMO_FOCUS_STAT_"):]
        short = "N" if short == "N_ROWS" else short
        assert getattr(abi, "FOCUS_" + short) == col == getattr(fr, short), name


def test_library_exports_both_entries():
    lib = abi.load_engine()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


def test_resident_rows_entry_refuses_without_a_result():
    """bmo_result_psf_rows, through which EngineSolution gets the rows of the through-focus read-outs: declared, exported, and a null
    result or null outputs are BMO_ERR_INVALID before anything is touched."""
    lib = abi.load_engine()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmo.h")).read(), flags=re.S)
    m = re.search(r"\bint bmo_result_psf_rows\((.*?)\);", hdr, flags=re.S)
    assert m and len(m.group(1).split(",")) == 5 == len(lib.bmo_result_psf_rows.argtypes)
    p, cnt, dev = C.POINTER(C.c_double)(), C.c_int64(), C.c_int32()
    assert lib.bmo_result_psf_rows(None, 0, C.byref(p), C.byref(cnt), C.byref(dev)) == INVALID
    assert b"bmo_result_psf_rows" in lib.bmo_last_error()
    sol = bmo.system.EngineSolution(lib, None, 1, 0)
    with pytest.raises(RuntimeError, match="bmo_result_psf_rows"):
        sol.psf_focus_stats(0, np.zeros(3), np.eye(3), [0.0])
    with pytest.raises(RuntimeError, match="bmo_result_psf_rows"):
        sol.psf_through_focus(0, np.zeros(3), np.eye(3), [0.0], n=4)


def test_argtypes_have_the_declared_arity():
    lib = abi.load_engine()
    for name, arity in SYMBOLS.items():
        assert len(getattr(lib, name).argtypes) == arity, name
    assert "displacements" in inspect.signature(abi.psf_through_focus).parameters
    assert "offsets" in inspect.signature(abi.psf_focus_stats).parameters
    assert fr.source_focus_mp() in (8, 16) and fr.source_focus_stat_mp() >= 1


def _stack_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, disp=True, n_planes=2, xs=True, zs=True, n=3, out=True, field=False):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    d, ax, I, F = np.array([[0.0, 0.0, 0.0], [1e-4, 2e-4, -1e-4]]), np.linspace(-1e-5, 1e-5, 3), np.zeros(2 * 9), np.zeros(2 * 2 * 9)
    ptr = lambda a, on: a.ctypes.data_as(dp) if on else None  # noqa: E731
    return abi.load_engine().bmo_psf_through_focus(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2),
                                                   ptr(d, disp), n_planes, ptr(ax, xs), ptr(ax, zs), n, 0, ptr(I, out), ptr(F, field), None)


def _stats_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, axis=True, offsets=True, n_planes=2, stats=True):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    a, off, st = np.cross(v[1], v[2]), np.array([0.0, 1e-4]), np.zeros(2 * 12)
    ptr = lambda a_, on: a_.ctypes.data_as(dp) if on else None  # noqa: E731
    return abi.load_engine().bmo_psf_focus_stats(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2),
                                                 ptr(a, axis), ptr(off, offsets), n_planes, 0, ptr(st, stats), None)


def test_bad_arguments_are_refused_and_valid_ones_need_a_device():
    lib = abi.load_engine()
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(disp=False), dict(n_planes=0), dict(n_planes=-3),
               dict(xs=False), dict(zs=False), dict(n=0), dict(n=-1), dict(out=False)):
        assert _stack_rc(**kw) == INVALID, kw
        assert b"bmo_psf_through_focus" in lib.bmo_last_error()
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(axis=False), dict(offsets=False), dict(n_planes=0),
               dict(n_planes=-3), dict(stats=False)):
        assert _stats_rc(**kw) == INVALID, kw
        assert b"bmo_psf_focus_stats" in lib.bmo_last_error()
    want = NO_DEVICE if lib.bmo_device_count() == 0 else 0  # no CPU fallback: valid arguments get as far as looking for a device
    for kw in (dict(), dict(field=True), dict(hits=False, n_hits=0), dict(n_planes=1)):
        assert _stack_rc(**kw) == want, (kw, lib.bmo_last_error())
    for kw in (dict(), dict(hits=False, n_hits=0), dict(n_planes=1)):
        assert _stats_rc(**kw) == want, (kw, lib.bmo_last_error())
