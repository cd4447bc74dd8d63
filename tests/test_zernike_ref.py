"""The yardsticks of the Zernike read-out tests, checked without a GPU: the basis against the closed forms, components.zernike_basis
against the helper bit for bit, the restated Cholesky and the a-posteriori bound (satisfiable, and with teeth), the exports, the refusals
that need no device, and the Julia constants."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import psf_stats_ref as pr
import zernike_ref as zr
from spot_ref import gamma

INVALID, NO_DEVICE = -1, -2


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def _polar_grid():
    rho = np.array([0.0, 0.05, 0.3, 0.5, 0.7071, 0.9, 0.999, 1.0])
    th = np.arange(12) * (2 * math.pi / 12) + 0.1
    return (rho[:, None] * np.cos(th)[None, :]).ravel(), (rho[:, None] * np.sin(th)[None, :]).ravel()


def test_terms_are_in_osa_ansi_order():
    for order in range(7):
        t = zr.terms(order)
        assert len(t) == zr.n_terms(order) == abi.zernike_sizes(order)[0]
        assert [zr.term_index(n, m) for n, m in t] == list(range(len(t)))
        assert bmo.components.zernike_terms(order) == t
    assert zr.terms(2) == [(0, 0), (1, -1), (1, 1), (2, -2), (2, 0), (2, 2)]
    assert zr.radial(6, 0) == [-1, 12, -30, 20] and zr.radial(4, 0) == [1, -6, 6] and zr.radial(3, 1) == [-2, 3] and zr.radial(5, 5) == [1]
    assert bmo.components.zernike_radial(6, 2) == zr.radial(6, 2) == [6, -20, 15]


def test_basis_equals_the_closed_forms():
    """Z_2^0 = sqrt 3 (2 rho^2 - 1), Z_4^0 = sqrt 5 (6 rho^4 - 6 rho^2 + 1), Z_3^1 = sqrt 8 (3 rho^3 - 2 rho) cos theta = sqrt 8 (3 rho^2 - 2) x,
    Z_6^0 = sqrt 7 (20 rho^6 - 30 rho^4 + 12 rho^2 - 1), each evaluated exactly (Fractions of the doubles x, y; N the correctly rounded root)
    on a polar grid.  Bound of the helper's value, with P(t) = sum |q_s| t^s, K = (n - m) / 2: the computed t carries theta_2 (t^s: theta_2s),
    Horner 2 K roundings more, so the radial factor is off by gamma_{4K+1} P(t); every monomial of C_m / S_m passes at most 3 m roundings and
    their absolute sum is (|x| + |y|)^m; the two products and the rounding of N add 3:
        |Z^ - Z| <= gamma_{4K+3m+4} N P(t) (|x| + |y|)^m       (a few u of the term's size N P (|x| + |y|)^m)."""
    x, y = _polar_grid()
    Z = zr.basis(x, y, 6)
    closed = {(2, 0): lambda t, a, b: 2 * t - 1, (4, 0): lambda t, a, b: 6 * t * t - 6 * t + 1, (3, 1): lambda t, a, b: (3 * t - 2) * a,
              (6, 0): lambda t, a, b: 20 * t ** 3 - 30 * t * t + 12 * t - 1, (2, -2): lambda t, a, b: 2 * a * b, (1, -1): lambda t, a, b: b}
    worst = 0.0
    for (n, m), f in closed.items():
        am, K = abs(m), (n - abs(m)) // 2
        nrm = Fraction(math.sqrt(n + 1) if m == 0 else math.sqrt(2 * (n + 1)))
        q = zr.radial(n, am)
        for h in range(len(x)):
            a, b = Fraction(float(x[h])), Fraction(float(y[h]))
            t = a * a + b * b
            want = nrm * f(t, a, b)
            size = nrm * sum(abs(c) * t ** s for s, c in enumerate(q)) * (abs(a) + abs(b)) ** am
            err = abs(Fraction(float(Z[zr.term_index(n, m), h])) - want)
            assert err <= gamma(4 * K + 3 * am + 4) * size, (n, m, h, float(err), float(size))
            if size:
                worst = max(worst, float(err / size) * 2 ** 53)
    print("largest error: %.2f u of the term size" % worst)
    assert np.all(Z[0] == 1.0)
    # orthonormal over the uniform disc: the Gram matrix of 5 000 random points is well conditioned
    rng = np.random.default_rng(5)
    r, th = np.sqrt(rng.uniform(0, 1, 5000)), rng.uniform(0, 2 * math.pi, 5000)
    B = zr.basis(r * np.cos(th), r * np.sin(th), 6)
    assert np.linalg.cond(B @ B.T / 5000) < 3


def test_components_basis_equals_the_helper_bit_for_bit():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-1, 1, 400), rng.uniform(-1, 1, 400)
    for order in range(7):
        a, b = bmo.components.zernike_basis(x, y, order), zr.basis(x, y, order)
        assert a.shape == (zr.n_terms(order), 400) and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert bmo.components.zernike_basis(0.25, -0.5, 3).shape == (10,)
    surf = bmo.components.zernike_surface([0.0, 0.0, 0.0, 0.0, 1e-8, 0.0], 9, 2)
    assert surf.shape == (9, 9) and np.isnan(surf[0, 0]) and surf[4, 4] == -math.sqrt(3.0) * 1e-8 and abs(surf[8, 4] - math.sqrt(3.0) * 1e-8) < 1e-23


def _host_fit(rows, pose, order, pupil=None):
    """A plain float64 evaluation of the read-out on the host (sequential sums): (coef, info, gram, proj, B)."""
    x, z = pr.local_xz(rows, *pose)
    w = rows[:, 7]
    u, v = zr.cosines(rows, pose[1], pose[2])
    info = np.full(zr.INFO_N, np.nan)
    s = float(np.cumsum(w)[-1])
    info[zr.N], info[zr.S] = len(rows), s
    info[zr.X_REF], info[zr.Z_REF] = np.cumsum(w * x)[-1] / s, np.cumsum(w * z)[-1] / s
    if pupil is None:
        info[zr.U0], info[zr.V0] = np.cumsum(w * u)[-1] / s, np.cumsum(w * v)[-1] / s
        info[zr.RHO] = np.sqrt(((u - info[zr.U0]) * (u - info[zr.U0]) + (v - info[zr.V0]) * (v - info[zr.V0])).max())
    else:
        info[zr.U0], info[zr.V0], info[zr.RHO] = pupil
    W = pr.paths(rows, pr.ref_point(*pose, info[zr.X_REF], info[zr.Z_REF]))
    info[zr.W_MEAN] = np.cumsum(w * W)[-1] / s
    proj, B, _, _ = zr.columns(rows, pose, info, order)
    J = zr.n_terms(order)
    gram = np.array([np.cumsum((proj * B[i]) * B[k])[-1] for i in range(J + 1) for k in range(i + 1)])
    coef, status, L = zr.cholesky_solve(gram, J)
    info[zr.STATUS] = status
    return np.array(coef), info, gram, proj, B, L


@pytest.mark.parametrize("n,order", [(300, 6), (2000, 2)])
def test_restated_cholesky_is_inside_the_a_posteriori_bound(pose, n, order):
    """The host evaluation is inside every bound (satisfiable), numpy.linalg.solve of the same normal equations agrees with the restated
    Cholesky within the sum of the two a-posteriori bounds (numpy's from its exact residual r = G^ c_np - b^:
    c_np - c = G^-1 (r + (b^ - b) - (G^ - G) c_np)), and a coefficient moved by 1e-6 of the largest one is caught."""
    rows = pr.synthetic_rows(n, 40 + n, pose)
    J = zr.n_terms(order)
    coef, info, gram, proj, B, L = _host_fit(rows, pose, order)
    assert info[zr.STATUS] == 0
    G, A = zr.exact_gram(proj, B)
    assert zr.gram_violations(gram, G, A, n) == []
    c, bound, Ginv = zr.coef_bounds(gram, G, J, coef, L)
    assert zr.coef_violations(coef, c, bound) == []
    big = max(abs(float(v)) for v in c)
    print("n = %d, order %d: largest |c| %.3g m, largest bound %.3g m" % (n, order, big, max(float(v) for v in bound)))
    assert max(float(v) for v in bound) < 1e-6 * big  # the bound has teeth
    # numpy.linalg.solve on the same doubles
    Gm = np.array([[gram[zr.packed(max(i, k), min(i, k))] for k in range(J)] for i in range(J)])
    bv = np.array([gram[zr.packed(J, k)] for k in range(J)])
    c_np = np.linalg.solve(Gm, bv)
    fr = lambda a: Fraction(float(a))  # noqa: E731
    rhs = []
    for q in range(J):
        r = sum(fr(Gm[q, k]) * fr(c_np[k]) for k in range(J)) - fr(bv[q])
        t = abs(r) + abs(fr(bv[q]) - G[zr.packed(J, q)])
        t += sum(abs(fr(Gm[q, k]) - G[zr.packed(max(q, k), min(q, k))]) * abs(fr(c_np[k])) for k in range(J))
        rhs.append(t)
    for i in range(J):
        b_np = sum(abs(Ginv[i][q]) * rhs[q] for q in range(J))
        assert b_np < 1e-6 * big
        assert abs(fr(c_np[i]) - fr(coef[i])) <= bound[i] + b_np, i
    # a coefficient moved by 1e-6 of the largest one
    moved = coef.copy()
    j = int(np.argmax(np.abs(coef)))
    moved[j] *= 1 + 1e-6
    assert [v[0] for v in zr.coef_violations(moved, c, bound)] == [j]
    moved = coef.copy()
    moved[J - 1] += 1e-6 * big
    assert [v[0] for v in zr.coef_violations(moved, c, bound)] == [J - 1]
    # and a Gram entry moved by 1e-9 of itself
    g2 = gram.copy()
    g2[zr.packed(J, 0) - 1] *= 1 + 1e-9
    assert len(zr.gram_violations(g2, G, A, n)) == 1


def test_fit_rms_bound_and_status_conventions(pose):
    rows = pr.synthetic_rows(64, 3, pose)
    coef, info, gram, proj, B, L = _host_fit(rows, pose, 2)
    E = zr.residual(B, coef)
    rms, b = zr.fit_rms_exact(proj, E)
    got = math.sqrt(float(np.cumsum(proj * (E * E))[-1]) / info[zr.S])
    assert abs(Fraction(got) - rms) <= b and b < 1e-9 * rms
    # a pivot that is not > 0: the restated Cholesky says STATUS 2 and NaN
    g = gram.copy()
    g[zr.packed(2, 2)] = 0.0
    c, status, _ = zr.cholesky_solve(g, 6)
    assert status == 2 and all(math.isnan(v) for v in c)


# ------------------------------------------------------------------------------------------------ exports and refusals that need no device
def _lib():
    return abi.load_engine()


def test_library_exports_both_entries():
    lib = _lib()
    for name in ("bmo_psf_zernike", "bmo_psf_zernike_sweep"):
        assert getattr(lib, name) is not None
    assert abi.ZERN_INFO_N == 13 and abi.ZERN_N_OUT == 12 and abi.ZERN_MAX_ORDER == 6
    assert abi.zernike_sizes(6) == (28, 435)


def _zern_rc(hits=True, n_hits=4, origin=True, e1=True, e2=True, ref=None, pupil=None, order=2, coef=True, info=True, gram=False):
    dp = C.POINTER(C.c_double)
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    r = None if ref is None else np.array(ref, dtype=np.float64)
    q = None if pupil is None else np.array(pupil, dtype=np.float64)
    cf, nf, gm = np.zeros(28), np.zeros(13), np.zeros(435)
    ptr = lambda a, on: a.ctypes.data_as(dp) if on else None  # noqa: E731
    return _lib().bmo_psf_zernike(rows.ctypes.data_as(C.c_void_p) if hits else None, n_hits, 0, ptr(v[0], origin), ptr(v[1], e1), ptr(v[2], e2),
                                  None if r is None else r.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), order, 0, ptr(cf, coef),
                                  ptr(nf, info), ptr(gm, gram), None)


def test_refusals_without_a_device():
    for kw in (dict(hits=False), dict(n_hits=-1), dict(origin=False), dict(e1=False), dict(e2=False), dict(coef=False), dict(info=False), dict(order=-1),
               dict(order=7), dict(pupil=(0.0, 0.0, 0.0)), dict(pupil=(0.0, 0.0, -0.03)), dict(pupil=(0.0, 0.0, math.inf)), dict(pupil=(0.0, 0.0, math.nan)),
               dict(pupil=(math.nan, 0.0, 0.03)), dict(pupil=(0.0, math.inf, 0.03))):
        assert _zern_rc(**kw) == INVALID, kw
        assert b"bmo_psf_zernike" in _lib().bmo_last_error()
    dp = C.POINTER(C.c_double)
    o, cf, nf = np.zeros(3), np.zeros(28), np.zeros(13)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    assert _lib().bmo_psf_zernike_sweep(None, 0, 1, p(o), p(o), p(o), None, None, 2, p(cf), p(nf), None, None) == INVALID
    assert b"bmo_psf_zernike_sweep" in _lib().bmo_last_error()


def test_valid_arguments_need_a_device():
    """No CPU fallback: with valid arguments the call gets as far as looking for a device."""
    for kw in (dict(), dict(ref=(1e-4, 0.0)), dict(pupil=(0.0, 0.01, 0.04), gram=True), dict(hits=False, n_hits=0), dict(order=0), dict(order=6)):
        rc = _zern_rc(**kw)
        assert rc == (NO_DEVICE if _lib().bmo_device_count() == 0 else 0), (kw, _lib().bmo_last_error())


# ------------------------------------------------------------------------------------------------ the Julia binding
def test_julia_constants_equal_the_enum():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "bmo.h")).read(), flags=re.S)
    body = re.search(r"enum bmo_zernike_info \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.strip(): int(v) for k, v in (item.split("=") for item in body.split(",") if item.strip())}
    assert len(enum) == 13 and sorted(enum.values()) == list(range(13))
    assert int(re.search(r"#define BMO_ZERNIKE_INFO_N (\d+)", hdr).group(1)) == 13 == abi.ZERN_INFO_N == zr.INFO_N
    assert int(re.search(r"#define BMO_ZERNIKE_MAX_ORDER (\d+)", hdr).group(1)) == 6 == abi.ZERN_MAX_ORDER
    jl = open(os.path.join(root, "julia", "GPUSystem.jl")).read()
    m = re.search(r"^const (ZERNIKE_N_ROWS[A-Z_0-9, ]+?) = Int32\.\((\d+):(\d+)\)$", jl, flags=re.M)
    names = [n.strip() for n in m.group(1).split(",")]
    assert (int(m.group(2)), int(m.group(3))) == (0, 12) and len(names) == 13
    for i, name in enumerate(names):
        assert enum["BMO_" + name] == i, name
        short = name[len("ZERNIKE_"):] if name != "ZERNIKE_N_ROWS" else "N"
        assert getattr(zr, short) == i and getattr(abi, "ZERN_" + short) == i, name
    assert re.search(r"^const ZERNIKE_INFO_N = Int32\(13\)$", jl, flags=re.M) and re.search(r"^const ZERNIKE_MAX_ORDER = Int32\(6\)$", jl, flags=re.M)
    for sym in ("bmo_psf_zernike", "bmo_psf_zernike_sweep"):
        assert "ccall((:%s, LIBBMO)" % sym in jl
