"""The yardsticks of the MTF read-out tests, checked without a GPU: the exact evaluators of tests/mtf_ref.py against closed forms, planted
mistakes that each miss a known answer by far more than a bound, the sampling rule of components.mtf_window on the Airy scene (oracle rows,
transform in numpy), the helpers of components.py, and the declarations, exports and refusals that need no device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import mtf_ref as mr
import psf_stats_ref as pr

cp = bmo.components
INVALID, NO_DEVICE = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = ([0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0])  # origin, e1, e2, axis: the plane y = 0, rows along +y


def _rows_at(points, weights):
    """Rows on the plane y = 0 that run along +y: they stand at the same (x, z) on every plane."""
    rows = np.zeros((len(points), 9))
    for r, (x, z), w in zip(rows, points, weights):
        r[:] = [x, 0.0, z, 0.0, 1.0, 0.0, 1.0, w, 2 * math.pi / 1e-6]
    return rows


A, F0 = 2.0 ** -16, 2.0 ** 13  # 15.3 um and 8 192 cycles/m: binary fractions, f a = 1 / 8 exactly


def _two_row_mtf(freqs, mistake=None, points=((-A, 0.0), (A, 0.0))):
    T, S, _ = mr.geo_otf_exact(_rows_at(points, [0.5, 0.5]), *FRAME, [0.0, 0.25], freqs, mistake=mistake)
    return np.abs(T) / S


def test_two_equal_rows_give_a_cosine():
    """Rows at x = -a and +a of equal weight: T = 2 w cos(2 pi fx a), MTF = |cos 2 pi fx a|, on every plane and whatever fz."""
    import mpmath as mp

    freqs = [[0.0, 0.0], [F0, 0.0], [2 * F0, 0.0], [3 * F0, 5e4], [4 * F0, -3e4], [12345.678, 1.0]]
    got = _two_row_mtf(freqs)
    with mp.workdps(40):
        want = [float(abs(mp.cospi(2 * mp.mpf(f[0]) * mp.mpf(A)))) for f in freqs]
    assert got.shape == (2, 6)
    for m in range(2):
        assert np.abs(got[m] - want).max() <= 2 * mr.U
    assert got[0, 0] == 1.0 and abs(got[0, 1] - math.sqrt(0.5)) <= 2 * mr.U and got[0, 2] <= mr.U and got[0, 4] == 1.0


def test_a_constant_image_gives_the_dirichlet_kernel():
    """I = 1 on n x n samples of pitch dx centred on 0: T(fx, 0) = n sin(pi fx n dx) / sin(pi fx dx)."""
    import mpmath as mp

    n, dx = 9, 2.0 ** -18
    xs = (np.arange(n) - (n - 1) / 2) * dx
    freqs = [[0.0, 0.0], [1000.0, 0.0], [2.0 ** 14, 0.0], [0.0, 2.0 ** 14], [31234.5, 0.0]]
    T, total = mr.otf_exact(np.ones((n, n)), xs, xs, freqs)
    assert total == n * n
    with mp.workdps(40):
        for q, f in enumerate(freqs):
            t = mp.mpf(max(f)) * mp.mpf(dx)
            want = n * (mp.sinpi(n * t) / mp.sinpi(t) if t else n)
            assert abs(T[q] - complex(want)) <= 2 * mr.U * n * n, (f, T[q], want)


def test_the_mtf_does_not_depend_on_the_centres():
    pose = pr.tilted_pose()
    rows = pr.synthetic_rows(12, 7, pose)
    axis, offs, freqs = np.cross(pose[1], pose[2]), [0.0, 2e-4], [[3e4, -2e4], [5e3, 6e4]]
    T0, S, _ = mr.geo_otf_exact(rows, *pose, axis, offs, freqs)
    T1, _, scales = mr.geo_otf_exact(rows, *pose, axis, offs, freqs, centers=[[3e-4, -2e-4], [1e-3, 5e-4]])
    assert np.abs(T0 - T1).max() > 1e-3 * S  # the phase does
    assert np.abs(np.abs(T0) - np.abs(T1)).max() <= 4 * mr.U * S
    assert scales[0][0] < 2e-6 and scales[1][0] > 1e-4  # about its centre the focused plane is a micrometre wide


@pytest.mark.parametrize("mistake,freq", [("pi_for_2pi", [2 * F0, 0.0]), ("swap_fx_fz", [2 * F0, 0.0]), ("n_for_s", [0.0, 0.0]), ("cycles_per_mm", [2 * F0, 0.0])])
def test_planted_mistakes_miss_the_known_answer(mistake, freq):
    """At fx a = 1 / 4 the two rows cancel: MTF = 0.  pi for 2 pi reads cos(pi / 4); fx and fz swapped on this spot (no extent in z) reads 1;
    cycles per millimetre reads cos(pi / 2000).  N for S at f = 0 (weights 0.5): 1 / 2 instead of 1.  The bounds are of the order 1e-12."""
    right, wrong = _two_row_mtf([freq])[0, 0], _two_row_mtf([freq], mistake=mistake)[0, 0]
    want = 1.0 if mistake == "n_for_s" else 0.0
    bound = mr.mtf_bound(mr.geo_bound(2, 1.0, 1e-18, (A, 0.0), freq), 1.0, 1.0, 2)
    assert abs(right - want) <= bound < 1e-12
    assert abs(wrong - want) > 0.4, (mistake, wrong)
    # the transform's evaluator shares the convention: a two-sample image at -a and +a
    img = np.array([[0.5], [0.5]])
    T, tot = mr.otf_exact(img, [-A, A], [0.0], [freq], mistake=mistake)
    assert abs(abs(T[0]) / tot - wrong) <= 4 * mr.U


def test_the_bounds_are_small_and_grow_with_the_frequency():
    b1, b2 = mr.geo_bound(600, 600.0, 3e-16, (1e-4, 1e-4), (5e4, 5e4)), mr.geo_bound(600, 600.0, 3e-16, (1e-4, 1e-4), (5e3, 5e3))
    assert 0 < b2 < b1 < 1e-9 * 600.0
    assert 0 < mr.otf_bound(1.0, np.linspace(-1e-4, 1e-4, 17), np.linspace(-1e-4, 1e-4, 17), (5e4, 5e4)) < 1e-13


# ------------------------------------------------------------------------------------------------ the helpers of components.py
def test_helpers():
    f = cp.mtf_frequencies(100.0, 5, 90.0)
    assert f.shape == (5, 2) and np.allclose(f[:, 1], [0, 25, 50, 75, 100]) and np.abs(f[:, 0]).max() < 1e-13
    assert np.array_equal(cp.mtf_frequencies(100.0, 3), [[0.0, 0.0], [50.0, 0.0], [100.0, 0.0]])
    lam, na = 1e-6, 0.0375
    assert abs(cp.mtf_cutoff(2 * math.pi / lam, na) - 2 * na / lam) < 1e-9 * 2 * na / lam
    lim = cp.mtf_diffraction_limit([0.0, 0.5, 1.0, 1.2, -0.5])
    assert lim[0] == 1.0 and abs(lim[1] - 2 / math.pi * (math.acos(0.5) - 0.5 * math.sqrt(0.75))) < 1e-15 and lim[2] == 0 and lim[3] == 0 and lim[4] == lim[1]
    k = 2 * math.pi / lam
    airy = 1.22 * math.pi / (k * na)
    for H, want_airy in ((300, 0.35 * 16.0), (1000, 10.0), (4000, 10.0)):  # L = 16, 29, 58 Airy radii: 0.35 L = 5.6, 10.2, 20.4
        hw, n = cp.mtf_window(k, na, H, 75e3, airy_radii=10)
        assert abs(hw / airy - want_airy) < 0.05 * want_airy, (H, hw / airy)
        assert 2 * hw / (n - 1) <= 0.75 / (2 * 75e3) < 2 * hw / (n - 2)
    assert cp.mtf_window(k, na, 4000, 75e3, airy_radii=24)[0] < 24 * airy  # capped by the replicas
    with pytest.raises(ValueError):
        cp.mtf_window(k, 0.0, 100, 75e3)
    xs = np.linspace(-1e-4, 1e-4, 21)  # pitch 10 um: Nyquist 5e4
    cp.mtf_check_pitch(xs, xs, [[4.9e4, -4.9e4]])
    with pytest.raises(ValueError, match="alias"):
        cp.mtf_check_pitch(xs, xs, [[0.0, 0.0], [5.1e4, 0.0]])
    with pytest.raises(ValueError, match="alias"):
        cp.mtf_check_pitch(xs, xs, [[0.0, -5.1e4]])
    with pytest.raises(ValueError, match="kind"):
        cp.psf_mtf(None, None, None, None, np.eye(3), [[0.0, 0.0]], kind="both")
    with pytest.raises(ValueError, match="finite"):
        cp.psf_mtf(None, None, None, None, np.eye(3), [[math.inf, 0.0]])


# ------------------------------------------------------------------------------------------------ the sampling rule on the Airy scene
def test_airy_scene_reaches_the_diffraction_limit(oracle):
    """The Airy KAT's scene at H = 1000 rays, window of 10 Airy radii about the centroid, n = 96: the MTF of the oracle's image, transformed
    in numpy, against 2 / pi (acos s - s sqrt(1 - s^2)) on both axes: within 0.02 up to the cutoff and 1e-3 beyond it up to 1.2 cutoffs.
    Measured here on 61 frequencies per axis: 0.0140 up to the cutoff (at 0.02 cutoffs: the tails the window cuts off), 3.8e-4 beyond; on 25
    frequencies per axis, steps of 0.05 cutoffs, which pass over that maximum: 0.0117 and 1.5e-4.  Cutoff 75 091 cycles/m against
    D / (lambda f) = 75 000.  A window of 16 Airy radii at n = 128 (above 0.35 L: the replicas of 1000 plane waves stand at 29) misses by
    0.25 on this frequency grid, which the rule avoids.  The geometric MTF reads 0.941 at half the cutoff and 0.916 at 0.6 cutoffs."""
    from test_psf_readout import airy_setup

    system, cs, psfd, lam, D = airy_setup(num_rays=1000)
    oracle.solve_system(system, cs)
    rows, pos, o = psfd.data, np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
    e1, e2 = o[:, 0], o[:, 2]
    assert len(rows) == 1000
    k, rho = float(rows[:, 8].max()), mr.pupil_rho(rows, e1, e2)
    f_c = cp.mtf_cutoff(k, rho)
    print("cutoff %.1f cycles/m, D / (lambda f) = %.1f" % (f_c, D / (lam * 200e-3)))
    assert abs(f_c - 75000.0) < 200.0
    airy = 1.22 * math.pi / (k * rho)
    hw, n_rule = cp.mtf_window(k, rho, len(rows), 1.2 * f_c, airy_radii=10)
    assert abs(hw - 10 * airy) < 1e-12 and n_rule <= 96
    loc, w = cp.psf_local_pos(rows, pos, o), rows[:, 7]
    cx, cz = (w * loc[:, 0]).sum() / w.sum(), (w * loc[:, 1]).sum() / w.sum()

    def worst(half_width, n):
        xs, zs = bmo.linalg.linrange(-half_width, half_width, n), bmo.linalg.linrange(-half_width, half_width, n)
        I = oracle.psf_intensity(rows, pos, e1, e2, cx + xs, cz + zs)[0]
        inside, beyond = 0.0, 0.0
        for az in (0.0, 90.0):
            fq = cp.mtf_frequencies(1.2 * f_c, 61, az)
            cp.mtf_check_pitch(xs, zs, fq)
            mtf, _ = mr.otf_numpy(I, xs, zs, fq)
            s = np.hypot(fq[:, 0], fq[:, 1]) / f_c
            err = np.abs(mtf - cp.mtf_diffraction_limit(s))
            inside, beyond = max(inside, err[s <= 1].max()), max(beyond, err[s > 1].max())
        return inside, beyond

    inside, beyond = worst(hw, 96)
    print("half width 10 Airy radii, n = 96: |MTF - limit| %.4f up to the cutoff, %.2e beyond" % (inside, beyond))
    assert inside <= 0.02 and beyond <= 1e-3
    wide, _ = worst(16 * airy, 128)
    print("half width 16 Airy radii, n = 128 (above the replica distance): %.3f" % wide)
    assert wide > 0.05  # what mtf_window's 0.35 L keeps out
    # the geometric MTF of the same rows: a spot of RMS radius r reads 1 - pi^2 f^2 r^2 to second order in f r (exp(-pi^2 f^2 r^2) for a
    # Gaussian one); the next order is below (pi f r)^4 / 2 = 2e-3 here
    rms_r = math.sqrt((w * ((loc[:, 0] - cx) ** 2 + (loc[:, 1] - cz) ** 2)).sum() / w.sum())
    for f in (f_c / 2, 0.6 * f_c):
        g = abs((w * np.exp(-2j * np.pi * f * (loc[:, 0] - cx))).sum()) / w.sum()
        print("geometric MTF at %.1f cutoffs: %.4f (RMS radius %.3e m: exp(-(pi f r)^2) = %.4f)" % (f / f_c, g, rms_r, math.exp(-(math.pi * f * rms_r) ** 2)))
        assert abs(g - math.exp(-(math.pi * f * rms_r) ** 2)) < 5e-3
    T, S, _ = mr.geo_otf_exact(rows[::10], pos, e1, e2, o[:, 1], [0.0], [[f_c / 2, 0.0]], centers=[[cx, cz]])
    g10 = abs((w[::10] * np.exp(-2j * np.pi * f_c / 2 * (loc[::10, 0] - cx))).sum())
    assert abs(abs(T[0, 0]) - g10) < 1e-9 * S  # the exact evaluator on every tenth row against numpy on the recorded positions


# ------------------------------------------------------------------------------------------------ declarations, exports, refusals
SYMBOLS = {"bmo_psf_geo_otf": 17, "bmo_psf_otf": 19}


def test_header_declares_both_entries_and_the_library_exports_them():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmo.h")).read(), flags=re.S)
    lib = abi.load_engine()
    for name, arity in SYMBOLS.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(getattr(lib, name).argtypes), name
    assert "centers" in inspect.signature(abi.psf_geo_otf).parameters and "freqs" in inspect.signature(abi.psf_otf).parameters
    for owner, name in ((bmo.PSFDetector, "mtf"), (bmo.system.EngineSolution, "psf_mtf")):
        p = inspect.signature(getattr(owner, name)).parameters
        assert all(q in p for q in ("freqs", "offsets", "kind", "n", "half_width", "axis", "follow")), name


def _geo_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, axis=True, offsets=True, centers=False, n_planes=2, freqs=True, n_freqs=3, otf=True, mtf=True,
            sums=True, bad_freq=None):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    a, off, cen = np.cross(v[1], v[2]), np.array([0.0, 1e-4]), np.zeros((2, 2))
    fq = np.array([[0.0, 0.0], [1e4, 0.0], [0.0, -2e4]])
    if bad_freq is not None:
        fq[2, 1] = bad_freq
    o_, m_, s_ = np.zeros(2 * 3 * 2), np.zeros(2 * 3), np.zeros(2)
    ptr = lambda a_, on: a_.ctypes.data_as(dp) if on else None  # noqa: E731
    return abi.load_engine().bmo_psf_geo_otf(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2), ptr(a, axis),
                                             ptr(off, offsets), ptr(cen, centers), n_planes, ptr(fq, freqs), n_freqs, 0, ptr(o_, otf), ptr(m_, mtf), ptr(s_, sums), None)


def _otf_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, disp=True, n_planes=2, xs=True, zs=True, n=3, freqs=True, n_freqs=3, otf=True, mtf=True, sums=True,
            img=False, bad_freq=None):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    d, ax, I = np.array([[0.0, 0.0, 0.0], [1e-4, 2e-4, -1e-4]]), np.linspace(-1e-5, 1e-5, 3), np.zeros(2 * 9)
    fq = np.array([[0.0, 0.0], [1e4, 0.0], [0.0, -2e4]])
    if bad_freq is not None:
        fq[1, 0] = bad_freq
    o_, m_, s_ = np.zeros(2 * 3 * 2), np.zeros(2 * 3), np.zeros(2)
    ptr = lambda a_, on: a_.ctypes.data_as(dp) if on else None  # noqa: E731
    return abi.load_engine().bmo_psf_otf(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2), ptr(d, disp),
                                         n_planes, ptr(ax, xs), ptr(ax, zs), n, ptr(fq, freqs), n_freqs, 0, ptr(o_, otf), ptr(m_, mtf), ptr(s_, sums), ptr(I, img), None)


def test_bad_arguments_are_refused_and_valid_ones_need_a_device():
    lib = abi.load_engine()
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(axis=False), dict(offsets=False), dict(n_planes=0),
               dict(n_planes=-3), dict(freqs=False), dict(n_freqs=0), dict(n_freqs=-1), dict(otf=False), dict(mtf=False), dict(sums=False), dict(bad_freq=math.nan),
               dict(bad_freq=math.inf)):
        assert _geo_rc(**kw) == INVALID, kw
        assert b"bmo_psf_geo_otf" in lib.bmo_last_error()
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(disp=False), dict(n_planes=0), dict(xs=False), dict(zs=False),
               dict(n=0), dict(n=-1), dict(freqs=False), dict(n_freqs=0), dict(otf=False), dict(mtf=False), dict(sums=False), dict(bad_freq=-math.inf),
               dict(bad_freq=math.nan)):
        assert _otf_rc(**kw) == INVALID, kw
        assert b"bmo_psf_otf" in lib.bmo_last_error()
    want = NO_DEVICE if lib.bmo_device_count() == 0 else 0  # no CPU fallback: valid arguments get as far as looking for a device
    for kw in (dict(), dict(centers=True), dict(hits=False, n_hits=0), dict(n_planes=1, n_freqs=1)):
        assert _geo_rc(**kw) == want, (kw, lib.bmo_last_error())
    for kw in (dict(), dict(img=True), dict(hits=False, n_hits=0), dict(n_planes=1, n_freqs=1)):
        assert _otf_rc(**kw) == want, (kw, lib.bmo_last_error())


def test_resident_rows_go_through_the_library():
    sol = bmo.system.EngineSolution(abi.load_engine(), None, 1, 0)
    for kind in ("diffraction", "geometric"):
        with pytest.raises(RuntimeError, match="bmo_result_psf_rows"):
            sol.psf_mtf(0, np.zeros(3), np.eye(3), [[0.0, 0.0]], kind=kind, half_width=1e-4)
