"""The yardsticks of the Spotdetector read-out tests, checked without a GPU: the numpy binning rule against exact arithmetic, the derived
statistics bounds against a plain two-pass evaluation (satisfiable) and the one-pass form (they have teeth), and the refusals of the four
entry points that need no device."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from bmo_amd import abi
import spot_ref as sr

mm = 1e-3
WINDOWS = [(-2.5 * mm, 2.5 * mm, -2.5 * mm, 2.5 * mm), (0.1 * mm, 0.7 * mm, -3.0 * mm, 1.3 * mm)]
SHAPES = [(1, 1), (7, 3), (1, 33), (300, 1), (128, 128), (129, 128)]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numpy_rule_agrees_with_exact_classification(seed):
    n = 2000
    set_aside = total = 0
    for window in WINDOWS:
        rows = sr.window_rows(n, window, seed)
        for nx, nz in SHAPES:
            want = np.zeros((nx, nz), dtype=np.int64)
            outside = 0
            ambiguous = []
            for r, (x, z) in enumerate(rows[:, :2].tolist()):
                e = sr.bin_exact(x, z, window, nx, nz)
                if e is None:
                    outside += 1
                    continue
                i, j, tx, tz = e
                if min(abs(tx - round(tx)), abs(tz - round(tz))) < Fraction(1, 10 ** 9):
                    ambiguous.append(r)
                    continue
                want[i, j] += 1
            total += n
            set_aside += len(ambiguous)
            keep = np.ones(n, dtype=bool)
            keep[ambiguous] = False
            got, got_out = sr.bin_rule(rows[keep], window, nx, nz)
            assert got_out == outside, (window, nx, nz)
            assert np.array_equal(got, want), (window, nx, nz)
            # a row next to a bin edge still lands in one of the two bins that share it (and membership is exact everywhere)
            for r in ambiguous:
                g, o = sr.bin_rule(rows[r:r + 1], window, nx, nz)
                i, j, tx, tz = sr.bin_exact(rows[r, 0], rows[r, 1], window, nx, nz)
                assert o == 0 and g.sum() == 1
                gi, gj = (int(v[0]) for v in np.nonzero(g))
                assert abs(gi - i) <= 1 and abs(gj - j) <= 1, (rows[r], window, nx, nz)
            # the crafted rows: NaN, +-inf and the one-ulp neighbours are outside, the edges inside
            assert outside >= 8
    assert set_aside <= 0.01 * total, (set_aside, total)


STAT_INPUTS = [(n, s) for n in (1, 63, 64, 65, 255, 256, 257, 5000) for s in (5,)]


@pytest.mark.parametrize("n,seed", STAT_INPUTS)
def test_two_pass_evaluation_is_inside_every_bound(n, seed):
    rows = sr.finite_rows(n, seed)
    assert sr.stat_violations(sr.two_pass_sequential(rows), rows) == []


def test_bounds_hold_for_two_passes_and_catch_one_pass_on_the_offset_spot():
    rows = sr.offset_spot()
    ex = sr.exact_stats(rows)
    got = sr.two_pass_sequential(rows)
    assert sr.stat_violations(got, rows, ex) == []
    bad = got.copy()
    bad[sr.MXX] = sr.one_pass_mxx(rows)
    names = [v[0] for v in sr.stat_violations(bad, rows, ex)]
    assert names == ["MXX"], names
    # the bound is tight enough to matter: far below the moment itself
    assert float(sr.stat_bounds(ex)[sr.MXX]) < 1e-9 * float(ex["val"][sr.MXX])


def test_empty_and_single_row_conventions():
    empty = np.full(sr.STAT_N, np.nan)
    empty[sr.N] = 0
    assert sr.stat_violations(empty, np.zeros((0, 2))) == []
    assert sr.stat_violations(np.zeros(sr.STAT_N), np.zeros((0, 2))) != []
    one = sr.two_pass_sequential(np.array([[1.25e-3, -0.5e-3]]))
    assert not one[sr.MXX:].any() and not np.signbit(one[sr.MXX:]).any()


def test_spot_splits_restatement_matches_the_source():
    assert sr.source_spot_constants() == (sr.SPOT_MIN_SPLIT, sr.SPOT_MAX_SPLITS, sr.LDS_BINS)
    assert sr.spot_splits(0) == (1, 256) and sr.spot_splits(1) == (1, 256) and sr.spot_splits(2048) == (1, 2048)
    n = sr.smallest_ragged_three_splits()
    ns, per = sr.spot_splits(n)
    assert ns >= 3 and per % 256 == 0 and 0 < n - (ns - 1) * per < per
    for m in (1, 255, 257, 4096, 4097, 10 ** 6 + 1, 1 << 26):
        ns, per = sr.spot_splits(m)
        assert per % 256 == 0 and (ns - 1) * per < m <= ns * per and ns <= sr.SPOT_MAX_SPLITS
    assert 128 * 128 == sr.LDS_BINS < 129 * 128


# ------------------------------------------------------------------------------------------------ refusals that need no device
def _lib():
    return abi.load_engine()


def test_library_exports_the_four_entries():
    lib = _lib()
    for name in ("bmo_spot_image", "bmo_spot_image_sweep", "bmo_spot_stats", "bmo_spot_stats_sweep"):
        assert getattr(lib, name) is not None


def _image_rc(rows=True, n_rows=4, row_cols=2, window=(-1.0, 1.0, -1.0, 1.0), nx=4, nz=4, image=True, outside=True):
    lib = _lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r = np.zeros((4, 10))
    w = None if window is None else np.array(window, dtype=np.float64)
    img = np.zeros(max(nx, 1) * max(nz, 1), dtype=np.int64)
    out = C.c_int64()
    return lib.bmo_spot_image(r.ctypes.data_as(C.c_void_p) if rows else None, n_rows, row_cols, 0, None if w is None else w.ctypes.data_as(dp), nx, nz, 0,
                              img.ctypes.data_as(ip) if image else None, C.byref(out) if outside else None, None)


def test_image_refusals_without_a_device():
    INVALID = -1
    nan = float("nan")
    cases = [dict(rows=False), dict(window=None), dict(image=False), dict(outside=False), dict(nx=0), dict(nz=0), dict(nx=-3), dict(row_cols=1),
             dict(row_cols=10), dict(window=(1.0, 1.0, -1.0, 1.0)), dict(window=(1.0, -1.0, -1.0, 1.0)), dict(window=(-1.0, 1.0, 2.0, 2.0)),
             dict(window=(nan, 1.0, -1.0, 1.0)), dict(window=(-1.0, 1.0, -1.0, nan)), dict(window=(-1.0, float("inf"), -1.0, 1.0)),
             dict(n_rows=-1)]
    for kw in cases:
        assert _image_rc(**kw) == INVALID, kw
        assert b"bmo_spot_image" in _lib().bmo_last_error()


def test_stats_and_sweep_refusals_without_a_device():
    lib = _lib()
    INVALID = -1
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    r, st = np.zeros((4, 10)), np.zeros(12)
    rp, sp = r.ctypes.data_as(C.c_void_p), st.ctypes.data_as(dp)
    assert lib.bmo_spot_stats(None, 4, 2, 0, 0, sp, None) == INVALID
    assert lib.bmo_spot_stats(rp, 4, 2, 0, 0, None, None) == INVALID
    assert lib.bmo_spot_stats(rp, 4, 1, 0, 0, sp, None) == INVALID
    assert lib.bmo_spot_stats(rp, 4, 10, 0, 0, sp, None) == INVALID
    w, img, out = np.array([-1.0, 1, -1, 1]), np.zeros(16, dtype=np.int64), np.zeros(1, dtype=np.int64)
    assert lib.bmo_spot_image_sweep(None, 0, 1, w.ctypes.data_as(dp), 4, 4, img.ctypes.data_as(ip), out.ctypes.data_as(ip), None) == INVALID
    assert lib.bmo_spot_stats_sweep(None, 0, 1, sp, None) == INVALID
