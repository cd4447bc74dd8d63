"""The yardsticks of the encircled-energy read-out tests, checked without a GPU: the exact evaluators of tests/ee_ref.py against known
answers, planted mistakes that each miss a known answer by far more than a bound, the helpers of components.py, and the declarations,
exports and refusals that need no device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import ee_ref as er
import psf_stats_ref as pr

cp = bmo.components
INVALID, NO_DEVICE, LIMIT = -1, -2, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2.0 ** -10  # the unit of the hand-made cases: a binary fraction, so 3 B, 4 B and 5 B and their squares are exact


# ------------------------------------------------------------------------------------------------ known answers
H_DISC, A_DISC, C_DISC = 1600, 1e-3, (8e-4, -6e-4)  # the disc's centre lies a whole radius from the origin
# Granularity of a Fibonacci disc of H points: a circle about its centre cuts the sequence r_i = a sqrt((i + 1/2) / H) at one place, so the
# count is within one point, 1 / H.  A square's perimeter 8 R crosses cells of area pi a^2 / H; allowing every cell within twice the
# side sqrt(pi a^2 / H) of it to fall on the wrong side: 8 R * 2 a sqrt(pi / H) / (pi a^2) = 0.113 at R = a / 2.
TOL_CIRCLE = 1.0 / H_DISC
TOL_SQUARE = 8 * 0.5 * 2 * math.sqrt(math.pi / H_DISC) / math.pi


def _disc(radii, shape, mistake=None):
    rows = er.fibonacci_disc_rows(H_DISC, A_DISC, center=C_DISC, proj=0.5)
    return er.geo_ee_exact(rows, *er.FLAT_FRAME, er.FLAT_AXIS, [0.0, 2.5e-4], radii, centers=[C_DISC, C_DISC], shape=shape, mistake=mistake)


def test_a_uniform_disc_holds_the_area_share():
    """Encircled: (R / a)^2; ensquared, for a square inside the disc: 4 R^2 / (pi a^2); the same on both planes (the rows run along the
    axis).  S = H / 2, count = energy / proj."""
    radii = np.array([0.25, 0.5, 0.8, 1.0, 1.5]) * A_DISC
    ex = _disc(radii, er.CIRCLE)
    assert ex["S"] == 0.5 * H_DISC and ex["ee"].shape == (2, 5)
    want = np.minimum((radii / A_DISC) ** 2, 1.0)
    assert np.abs(ex["ee"] - want[None, :]).max() <= TOL_CIRCLE + 1e-15
    assert np.array_equal(ex["count"] * 0.5, ex["energy"]) and np.array_equal(ex["mass"], ex["energy"])
    assert ex["count"][0, 3] >= H_DISC - 1 and ex["count"][0, 4] == H_DISC  # the outermost point stands at a sqrt(1 - 1 / (2 H)) < a
    sq = _disc(radii[:2], er.SQUARE)
    want = 4 * radii[:2] ** 2 / (math.pi * A_DISC ** 2)
    print("ensquared", sq["ee"][0], "want", want)
    assert np.abs(sq["ee"] - want[None, :]).max() <= TOL_SQUARE


def _two_rows(shape, radii, mistake=None, center=(0.0, 0.0)):
    rows = np.zeros((2, 9))
    rows[0] = [3 * B + center[0], 0.0, 4 * B + center[1], 0.0, 1.0, 0.0, 1.0, 0.25, 2 * math.pi / 1e-6]
    rows[1] = [-6 * B + center[0], 0.0, 8 * B + center[1], 0.0, 1.0, 0.0, 1.0, 0.75, 2 * math.pi / 1e-6]
    return er.geo_ee_exact(rows, *er.FLAT_FRAME, er.FLAT_AXIS, [0.0], radii, centers=[center], shape=shape, mistake=mistake)


def test_two_rows_by_hand():
    """Rows at (3, 4) and (-6, 8) units with the weights 1/4 and 3/4: the first lies ON the circle of 5 units (9 + 16 = 25) and ON the square
    of 4 units, and the edge is closed."""
    ex = _two_rows(er.CIRCLE, [4.999 * B, 5 * B, 9.999 * B, 10 * B])
    assert ex["count"].tolist() == [[0, 1, 1, 2]] and ex["energy"].tolist() == [[0.0, 0.25, 0.25, 1.0]] and ex["ee"].tolist() == [[0.0, 0.25, 0.25, 1.0]]
    assert [float(k) for k in ex["keys"][0]] == [25 * B * B, 100 * B * B] and ex["A"] == [8 * B] and ex["S"] == 1.0
    ex = _two_rows(er.SQUARE, [3 * B, 4 * B, 7.5 * B, 8 * B])
    assert ex["count"].tolist() == [[0, 1, 1, 2]] and ex["ee"].tolist() == [[0.0, 0.25, 0.25, 1.0]]
    assert [float(k) for k in ex["keys"][0]] == [4 * B, 8 * B]
    assert er.gaps(ex["keys"][0], ex["thr"]) == [B, 0.0, 0.5 * B, 0.0]
    assert er.undecided(ex["keys"][0], ex["thr"], 0.0) == [(0, 1), (1, 3)] and er.undecided(ex["keys"][0], ex["thr"][:1], 0.5 * B) == []
    assert er.undecided(ex["keys"][0], ex["thr"], [B, 0.0, 0.0, 0.0]) == [(0, 0), (0, 1), (1, 3)]


def test_an_image_of_ones_by_hand():
    """5 x 5 samples of one on the integer grid, about the centre sample: the circle of one pitch holds 5 of them, the square 9; about a
    corner sample the circle of one pitch holds 3."""
    xs = (np.arange(5) - 2.0) * B
    I = np.ones((5, 5))
    ex = er.image_ee_exact(I, xs, xs, (0.0, 0.0), [0.0, B, 1.5 * B, 4 * B], shape=er.CIRCLE)
    assert ex["count"].tolist() == [1, 5, 9, 25] and ex["energy"].tolist() == [1.0, 5.0, 9.0, 25.0] and ex["S"] == 25.0 and ex["ee"][1] == 0.2
    assert ex["centroid"] == (0.0, 0.0) and ex["A"] == 2 * B and len(ex["keys"]) == 25
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B, 2 * B], shape=er.SQUARE)["count"].tolist() == [9, 25]
    assert er.image_ee_exact(I, xs, xs, (-2 * B, 2 * B), [B], shape=er.CIRCLE)["count"].tolist() == [3]
    I[4, 0] = 26.0  # a weight of 25 more at (2, -2) units: the centroid moves half way there
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], shape=er.CIRCLE)["centroid"] == (B, -B)


def test_every_planted_mistake_misses_a_known_answer():
    """Each mistake of ee_ref.MISTAKES against the known answer it spoils, by at least a hundred times the allowance of that answer."""
    half = [0.5 * A_DISC]
    missed = {}
    for mistake in ("r_for_r2", "n_for_s", "center_ignored"):
        missed[mistake] = abs(_disc(half, er.CIRCLE, mistake)["ee"][0, 0] - 0.25) / TOL_CIRCLE
    assert abs(_disc(half, er.CIRCLE)["ee"][0, 0] - 0.25) <= TOL_CIRCLE
    # the hand-made rows have exact answers: the allowance is the rounding of the result, u.  Row (3, 4) is outside the square of 3.5 units
    # (a test on x alone takes it in) and on the circle of 5 units (an open edge leaves it out).
    assert _two_rows(er.SQUARE, [3.5 * B])["ee"].tolist() == [[0.0]] and _two_rows(er.CIRCLE, [5 * B])["ee"].tolist() == [[0.25]]
    missed["square_one_axis"] = abs(_two_rows(er.SQUARE, [3.5 * B], "square_one_axis")["ee"][0, 0] - 0.0) / er.U
    missed["open_edge"] = abs(_two_rows(er.CIRCLE, [5 * B], "open_edge")["ee"][0, 0] - 0.25) / er.U
    print({k: "%.3g allowances" % v for k, v in missed.items()})
    assert set(missed) == set(er.MISTAKES)
    for mistake, ratio in missed.items():
        assert ratio >= 100, (mistake, ratio)
    # a strip |ax| <= a / 2 of the disc holds (2 / pi) (asin(1 / 2) + sqrt(3) / 4) = 0.609 of it, the square 1 / pi = 0.318
    assert abs(_disc(half, er.SQUARE, "square_one_axis")["ee"][0, 0] - 0.609) < 0.02
    assert _two_rows(er.SQUARE, [4 * B], "open_edge")["count"].tolist() == [[0]]
    assert _two_rows(er.CIRCLE, [5 * B], center=(7 * B, 0.0))["count"].tolist() == [[1]]
    assert _two_rows(er.CIRCLE, [5 * B], "center_ignored", center=(7 * B, 0.0))["count"].tolist() == [[0]]
    # the image evaluator: 5 x 5 samples of two, the circle of one pitch (5 samples, energy 10) or the square (9); about a corner, 3
    xs = (np.arange(5) - 2.0) * B
    I = 2 * np.ones((5, 5))
    corner = (-2 * B, 2 * B)
    right = er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B])
    assert right["count"].tolist() == [5] and right["energy"].tolist() == [10.0] and er.image_ee_exact(I, xs, xs, corner, [B])["count"].tolist() == [3]
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], mistake="open_edge")["count"].tolist() == [1]
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], mistake="r_for_r2")["count"].tolist() == [25]
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], mistake="n_for_s")["energy"].tolist() == [5.0]
    assert er.image_ee_exact(I, xs, xs, corner, [B], mistake="center_ignored")["count"].tolist() == [5]
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], shape=er.SQUARE)["count"].tolist() == [9]
    assert er.image_ee_exact(I, xs, xs, (0.0, 0.0), [B], shape=er.SQUARE, mistake="square_one_axis")["count"].tolist() == [15]


def test_the_decision_distance_and_the_bounds():
    """d_key by hand; the bounds scale as their derivation says."""
    u = er.U
    assert er.d_key(2.0, 3.0, er.SQUARE) == u * 2.0 * (1 + u)
    e_a = u * 2.0 * (1 + u)
    assert er.d_key(2.0, 3.0, er.CIRCLE) == 4 * 2.0 * e_a + 2 * e_a * e_a + 4 * u * 4.0 * (1 + u) + u * 9.0
    e_a = 1e-15 + u * (2.0 + 1e-15) * (1 + u)
    assert er.d_key(2.0, 3.0, er.SQUARE, e_row=1e-15) == e_a and er.d_key(2.0, 0.0, er.CIRCLE, e_row=1e-15) > 8 * 1e-15
    assert er.energy_bound(599, 10.0, 7.0) == er.fr.gamma(599) * 10.0 + u * 7.0
    assert er.ee_bound(599, 10.0, 7.0, 20.0, 0.35) >= er.energy_bound(599, 10.0, 7.0) / 20.0 + 600 * u * 0.35
    assert er.centroid_bound(17, 3.0, 2.0, 0.5) > er.fr.gamma(35) * 1.5 + er.fr.gamma(34) * 0.5


def test_radii_between_stand_in_the_widest_gap_nearby():
    import mpmath as mp

    keys = [mp.mpf(v) ** 2 for v in (1.0, 1.1, 1.3, 2.0, 2.05, 2.1, 3.0)]
    r = er.radii_between(keys, [0.0, 0.5, 1.0], er.CIRCLE, reach=1)
    assert np.allclose(r, [1.2, 1.65, 2.55], rtol=0, atol=1e-15)  # the gap of .2 beside the first, of .7 beside the middle, of .9 at the end
    assert np.allclose(er.radii_between([mp.sqrt(k) for k in keys], [0.5], er.SQUARE, reach=0), [2.025], rtol=0, atol=1e-15)
    with mp.workdps(40):
        assert min(er.gaps(keys, er.thresholds_exact(r, er.CIRCLE))) > 0.1


# ------------------------------------------------------------------------------------------------ the helpers of components.py
def test_diffraction_limit_against_mpmath():
    import mpmath as mp

    v = np.linspace(0.0, 30.0, 241)
    got = cp.ee_diffraction_limit(v)
    with mp.workdps(30):
        want = np.array([float(1 - mp.besselj(0, mp.mpf(float(t))) ** 2 - mp.besselj(1, mp.mpf(float(t))) ** 2) for t in v])
    print("largest error of ee_diffraction_limit on [0, 30]: %.3e" % np.abs(got - want).max())
    assert np.abs(got - want).max() <= 1e-12
    with mp.workdps(30):
        ring = mp.findroot(lambda t: mp.besselj(1, t), 3.83)  # the first dark ring holds 1 - J0^2 = 83.8 % of the light
        assert abs(float(cp.ee_diffraction_limit(float(ring))) - float(1 - mp.besselj(0, ring) ** 2)) < 1e-12 and abs(float(cp.ee_diffraction_limit(float(ring))) - 0.838) < 5e-4
    assert got[0] == 0.0
    assert cp.ee_diffraction_limit(np.zeros((2, 3))).shape == (2, 3)
    assert np.all(np.diff(got) >= -1e-15)


def test_radius_at_a_fraction():
    radii = [0.0, 1.0, 2.0, 4.0]
    assert abs(cp.ee_radius_at(radii, [0.0, 0.5, 0.75, 1.0], 0.8) - 2.4) < 1e-15
    assert cp.ee_radius_at(radii, [0.0, 0.5, 0.75, 1.0], 0.5) == 1.0 and cp.ee_radius_at(radii, [0.0, 0.5, 0.75, 1.0], 0.25) == 0.5
    assert cp.ee_radius_at(radii, [0.3, 0.5, 0.75, 1.0], 0.2) == 0.0  # the curve starts above: the first radius
    assert abs(cp.ee_radius_at(radii, [0.0, 0.9, 0.7, 1.0], 0.8) - 8 / 9) < 1e-15  # the FIRST crossing
    assert math.isnan(cp.ee_radius_at(radii, [0.0, 0.5, 0.75, 0.79], 0.8))  # not reached
    assert math.isnan(cp.ee_radius_at(radii, [math.nan] * 4, 0.8))
    both = cp.ee_radius_at(radii, [[0.0, 0.5, 0.75, 1.0], [0.0, 0.1, 0.2, 0.3]], 0.8)
    assert both.shape == (2,) and abs(both[0] - 2.4) < 1e-15 and math.isnan(both[1])
    with pytest.raises(ValueError, match="ascending"):
        cp.ee_radius_at([0.0, 2.0, 1.0], [0.0, 0.5, 1.0], 0.5)
    with pytest.raises(ValueError, match="one value per radius"):
        cp.ee_radius_at([0.0, 1.0], [0.0, 0.5, 1.0], 0.5)
    assert cp.ee_radii(3e-5, 4).tolist() == [0.0, 1e-5, 2e-5, 3e-5] and cp.ee_radii(2.0, 1).tolist() == [0.0]


def test_the_python_layer_refuses_what_it_cannot_read():
    def never(*a):
        raise AssertionError("the read-out must not be reached")

    drive = lambda **kw: cp.psf_encircled_energy(never, never, never, never, np.eye(3), **kw)  # noqa: E731
    for kw, match in ((dict(radii=[1e-5], kind="fourier"), "kind"), (dict(radii=[1e-5], shape="hexagon"), "shape"), (dict(radii=[1e-5], follow="chief"), "follow"),
                      (dict(radii=[]), "radius"), (dict(radii=[1e-5, -1e-6]), "radius"), (dict(radii=[math.nan]), "radius"), (dict(radii=[math.inf]), "radius"),
                      (dict(radii=[1e-5], offsets=[]), "offsets"),
                      (dict(radii=[1e-5, 2e-4], kind="diffraction", n=8, half_width=1e-4), "window"),
                      (dict(radii=[1.5e-4], kind="diffraction", shape="square", n=8, half_width=(2e-4, 1e-4)), "window")):
        with pytest.raises(ValueError, match=match):
            drive(**kw)
    psfd = bmo.PSFDetector(1e-2)
    with pytest.raises(ValueError, match="window"):
        psfd.encircled_energy([2e-4], kind="diffraction", n=8, half_width=1e-4)
    with pytest.raises(ValueError, match="shape"):
        abi.spot_ee(np.zeros((3, 2)), (0.0, 0.0), [1.0], shape="hexagon")
    # the window holds the radius but not the radius about the centroid the read-out found: refused once the centre is known
    st = np.zeros((1, abi.FOCUS_STAT_N))
    st[0, abi.FOCUS_N] = 5
    ee_fn = lambda d, xs, zs, r, sh: (np.ones((1, 1)), np.ones((1, 1)), np.ones(1), np.array([[0.0, 3e-5]]))  # noqa: E731
    with pytest.raises(ValueError, match="centroid of plane 0.*window"):
        cp.psf_encircled_energy(lambda ax, off: st, never, ee_fn, never, np.eye(3), [8e-5], kind="diffraction", n=8, half_width=1e-4)
    out = cp.psf_encircled_energy(lambda ax, off: st, never, ee_fn, never, np.eye(3), [7e-5], kind="diffraction", n=8, half_width=1e-4)
    assert out[0].shape == (1, 1) and out[3].tolist() == [[0.0, 3e-5]]
    assert np.isnan(cp.spot_ee_fraction([0, 0], 0)).all() and cp.spot_ee_fraction([[1, 2], [0, 0]], [4, 0])[0].tolist() == [0.25, 0.5]
    assert cp.spot_ee_centers([0.0] + [math.nan] * 11).tolist() == [0.0, 0.0] and cp.spot_ee_centers([2.0, 1.5, -2.5] + [0.0] * 9).tolist() == [1.5, -2.5]


# ------------------------------------------------------------------------------------------------ declarations, exports, refusals
SYMBOLS = {"bmo_spot_ee": 11, "bmo_spot_ee_sweep": 10, "bmo_psf_geo_ee": 19, "bmo_psf_ee": 22}


def test_header_declares_the_entries_and_the_library_exports_them():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bmo.h")).read(), flags=re.S)
    lib = abi.load_engine()
    for name, arity in SYMBOLS.items():
        m = re.search(r"\bint %s\((.*?)\);" % name, hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == arity == len(getattr(lib, name).argtypes), name
    for fn, names in ((abi.spot_ee, ("rows_device_ptr", "n_rows", "shape")), (abi.spot_ee_sweep, ("centers", "radii")),
                      (abi.psf_geo_ee, ("hits_device_ptr", "n_hits", "centers", "shape")), (abi.psf_ee, ("hits_device_ptr", "n_hits", "want_intensity", "centers"))):
        assert all(q in inspect.signature(fn).parameters for q in names), fn
    for owner, name in ((bmo.PSFDetector, "encircled_energy"), (bmo.system.EngineSolution, "psf_encircled_energy")):
        p = inspect.signature(getattr(owner, name)).parameters
        assert all(q in p for q in ("radii", "offsets", "kind", "shape", "n", "half_width", "axis", "follow")), name
        assert p["kind"].default == "geometric" and p["shape"].default == "circle" and p["offsets"].default == (0.0,)
    for owner, name in ((bmo.Spotdetector, "encircled_energy"), (bmo.system.EngineSolution, "spot_encircled_energy"), (bmo.system.SweepSolution, "spot_encircled_energy")):
        p = inspect.signature(getattr(owner, name)).parameters
        assert all(q in p for q in ("radii", "center", "shape")), name


_DP = C.POINTER(C.c_double)


def _call(name, over):
    """The entry `name` on four valid synthetic rows with the arguments named in `over` replaced (None: a null pointer)."""
    rows = pr.synthetic_rows(4, 1, pr.tilted_pose())
    v = [np.array(a, dtype=np.float64) for a in pr.tilted_pose()]
    keep = dict(origin=v[0], e1=v[1], e2=v[2], axis=np.cross(v[1], v[2]), offsets=np.array([0.0, 1e-4]), centers=np.zeros((2, 2)), center=np.zeros(2),
                radii=np.array([1e-5, 0.0, 3e-5]), disp=np.array([[0.0, 0.0, 0.0], [1e-4, 2e-4, -1e-4]]), xs=np.linspace(-1e-5, 1e-5, 3), zs=np.linspace(-1e-5, 1e-5, 3),
                ee=np.zeros(6), energy=np.zeros(6), count=np.zeros(6, dtype=np.int64), sums=np.zeros(2), centers_out=np.zeros(4), img=np.zeros(18),
                inside=np.zeros(3, dtype=np.int64))
    a = dict(hits=rows, n_hits=4, n_rows=4, row_cols=9, n_planes=2, n=3, shape=0, n_radii=3)
    a.update(keep)
    a.update(over)
    for k, val in a.items():
        if isinstance(val, np.ndarray):
            a[k] = val.ctypes.data_as(C.c_void_p if k == "hits" else C.POINTER(C.c_int64) if val.dtype == np.int64 else _DP)
    lib = abi.load_engine()
    if name == "bmo_spot_ee":
        return lib.bmo_spot_ee(a["hits"], a["n_rows"], a["row_cols"], 0, a["center"], a["shape"], a["radii"], a["n_radii"], 0, a["inside"], None)
    if name == "bmo_psf_geo_ee":
        return lib.bmo_psf_geo_ee(a["hits"], a["n_hits"], 0, a["origin"], a["e1"], a["e2"], a["axis"], a["offsets"], a["centers"], a["n_planes"], a["shape"], a["radii"],
                                  a["n_radii"], 0, a["ee"], a["energy"], a["count"], a["sums"], None)
    return lib.bmo_psf_ee(a["hits"], a["n_hits"], 0, a["origin"], a["e1"], a["e2"], a["disp"], a["n_planes"], a["xs"], a["zs"], a["n"], a["centers"], a["shape"], a["radii"],
                          a["n_radii"], 0, a["ee"], a["energy"], a["sums"], a["centers_out"], a["img"], None)


def _bad(k, value):
    r = np.array([1e-5, 0.0, 3e-5])
    r[k] = value
    return r


def test_bad_arguments_are_refused_and_valid_ones_need_a_device():
    lib = abi.load_engine()
    shared = [dict(hits=None), dict(n_radii=0), dict(n_radii=-2), dict(shape=-1), dict(shape=2), dict(radii=None), dict(radii=_bad(0, -1e-9)), dict(radii=_bad(2, math.nan)),
              dict(radii=_bad(1, math.inf))]
    psf = [dict(n_hits=-1), dict(origin=None), dict(e1=None), dict(e2=None), dict(n_planes=0), dict(n_planes=-3), dict(ee=None), dict(energy=None), dict(sums=None),
           dict(centers=np.array([[0.0, 0.0], [math.nan, 0.0]])), dict(centers=np.array([[0.0, -math.inf], [0.0, 0.0]]))]
    cases = {"bmo_spot_ee": shared + [dict(n_rows=-1), dict(center=None), dict(inside=None), dict(row_cols=1), dict(row_cols=10), dict(center=np.array([0.0, math.nan])),
                                       dict(center=np.array([math.inf, 0.0]))],
             "bmo_psf_geo_ee": shared + psf + [dict(axis=None), dict(offsets=None)],
             "bmo_psf_ee": shared + psf + [dict(disp=None), dict(xs=None), dict(zs=None), dict(n=0), dict(n=-1), dict(centers_out=None)]}
    for name, kws in cases.items():
        for kw in kws:
            assert _call(name, kw) == INVALID, (name, kw)
            assert name.encode() in lib.bmo_last_error()
    assert _call("bmo_spot_ee", dict(n_radii=4097, radii=np.zeros(4097), inside=np.zeros(4097, dtype=np.int64))) == LIMIT
    want = NO_DEVICE if lib.bmo_device_count() == 0 else 0  # no CPU fallback: valid arguments get as far as looking for a device
    for name, kws in (("bmo_spot_ee", [dict(), dict(hits=None, n_rows=0), dict(row_cols=2, n_rows=18), dict(shape=1)]),
                      ("bmo_psf_geo_ee", [dict(), dict(centers=None), dict(count=None), dict(hits=None, n_hits=0), dict(shape=1, n_planes=1, n_radii=1)]),
                      ("bmo_psf_ee", [dict(), dict(centers=None), dict(img=None), dict(hits=None, n_hits=0), dict(shape=1, n_planes=1, n_radii=1)])):
        for kw in kws:
            assert _call(name, kw) == want, (name, kw, lib.bmo_last_error())
    ip = C.POINTER(C.c_int64)
    out, nr, r, c = np.zeros(3, dtype=np.int64), np.zeros(1, dtype=np.int64), np.array([1e-5, 0.0, 3e-5]), np.zeros(2)
    for res, cen, rad, n_radii, ins, rows in ((None, c, r, 3, out, nr), (C.c_void_p(1), None, r, 3, out, nr), (C.c_void_p(1), c, None, 3, out, nr),
                                              (C.c_void_p(1), c, r, 0, out, nr), (C.c_void_p(1), c, r, 3, None, nr), (C.c_void_p(1), c, r, 3, out, None)):
        ptr = lambda a_, t: None if a_ is None else a_.ctypes.data_as(t)  # noqa: E731
        assert lib.bmo_spot_ee_sweep(res, 0, 1, ptr(cen, _DP), 0, ptr(rad, _DP), n_radii, ptr(ins, ip), ptr(rows, ip), None) == INVALID
        assert b"bmo_spot_ee_sweep" in lib.bmo_last_error()


def test_resident_rows_go_through_the_library():
    sol = bmo.system.EngineSolution(abi.load_engine(), None, 1, 0)
    for kind in ("diffraction", "geometric"):
        with pytest.raises(RuntimeError, match="bmo_result_psf_rows"):
            sol.psf_encircled_energy(0, np.zeros(3), np.eye(3), [1e-5], kind=kind, n=8, half_width=1e-4)
    with pytest.raises(RuntimeError, match=r"bmo_spot_ee_sweep failed \(-1\)"):
        sol.spot_encircled_energy(0, [1e-5], center=(0.0, 0.0))
