"""Wavefront read-out on the GPU: bmo_psf_stats against the exact statistics of the same per-row doubles, inside the derived bounds of
tests/psf_stats_ref.py (nothing fitted), on synthetic rows at the project's scales, on an analytic perfect focus, and against the field of
the existing PSF read-out."""
import ctypes as C
import math

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import psf_stats_ref as pr
import readout_ref as rr
import spot_ref as sr
from test_psf_readout import airy_setup

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 5000, sr.smallest_ragged_three_splits()]
GIVEN = (pr.F_LOCAL[0] + 2e-7, pr.F_LOCAL[1] - 1e-7)


@pytest.fixture(scope="module")
def pose():
    return pr.tilted_pose()


def same_bits(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _resident(rows, pose, ref):
    """the statistics of a copy of the rows in device memory"""
    hip = C.CDLL("libamdhip64.so")
    rows = np.ascontiguousarray(rows)
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(max(rows.nbytes, 8))) == 0
    try:
        assert hip.hipMemcpy(dptr, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0  # hipMemcpyHostToDevice
        return abi.psf_stats(None, *pose, ref=ref, hits_device_ptr=dptr.value, n_hits=len(rows))[0]
    finally:
        hip.hipFree(dptr)


def _report(tag, st):
    print("%s: N %d  S %.17g  C (%.17g, %.17g)  HW (%.3g, %.3g)  W_MEAN %.17g  W_RMS %.6g  PV %.6g  F (%.10g, %.10g)  STREHL %.17g"
          % (tag, st[pr.N], st[pr.S], st[pr.CX], st[pr.CZ], st[pr.HWX], st[pr.HWZ], st[pr.W_MEAN], st[pr.W_RMS], st[pr.W_HI] - st[pr.W_LO],
             st[pr.F_RE], st[pr.F_IM], st[pr.STREHL]))


@pytest.mark.parametrize("n", COUNTS)
def test_synthetic_rows_inside_every_bound(pose, n):
    if n > 5000:
        ns, per = sr.spot_splits(n)
        assert ns >= 3 and n % per  # three splits, the last one ragged
    rows = pr.synthetic_rows(n, 100 + n, pose)
    for ref in (None, GIVEN):
        st, ms = abi.psf_stats(rows, *pose, ref=ref)
        _report("n = %d, ref %s" % (n, ref), st)
        assert pr.stat_violations(st, rows, *pose, ref=ref) == [], (n, ref)
        assert same_bits(st, _resident(rows, pose, ref)), (n, ref)
        if n:
            assert ms > 0
            assert n == 1 or 1e-8 < st[pr.W_RMS] < 1e-7  # 10 - 100 nm of wavefront spread (one row has none)
            assert st[pr.K_MIN] == st[pr.K_MAX] and bmo.components.psf_marechal(st) == np.exp(-(st[pr.K_MIN] * st[pr.W_RMS]) ** 2)
            assert abs(st[pr.K_MIN] * st[pr.W_MEAN]) > 1.2e6  # phases of 1.3e6 rad
        else:
            assert st[pr.N] == 0 and np.isnan(st[1:]).all()


@pytest.mark.parametrize("n", [257, 5000])
def test_two_wavelengths_in_one_table(pose, n):
    rows = pr.synthetic_rows(n, 7, pose, two_wavelengths=True)
    st, _ = abi.psf_stats(rows, *pose)
    _report("two wavelengths, n = %d" % n, st)
    assert st[pr.K_MIN] < st[pr.K_MAX]
    assert math.isnan(bmo.components.psf_marechal(st))
    assert pr.stat_violations(st, rows, *pose) == []


@pytest.mark.parametrize("n", [300, 5000])
def test_perfect_focus(pose, n):
    """Rays of a sphere about f read at f: W_h = R up to the rounding E_row of the rows (psf_stats_ref.focus_row_error), so
    W_RMS <= E_row + its bound, every |W_h - W_MEAN^| <= (2 E_row + E_w)(1 + u), and with |F| >= sum proj cos(k (W_h - W_0)) >= S (1 - (k D)^2 / 2)
    for D = max |W_h - W_0| <= 2 E_row: STREHL >= (1 - (k D)^2 / 2)^2 >= 1 - (2 k E_row)^2, less its bound; it never exceeds 1 + its bound."""
    rows, f = pr.focus_rows(n, 21, pose)
    st, _ = abi.psf_stats(rows, *pose, ref=pr.F_LOCAL)
    _report("perfect focus, n = %d" % n, st)
    assert pr.stat_violations(st, rows, *pose, ref=pr.F_LOCAL) == []
    e_row = pr.focus_row_error(f)
    x, z = pr.local_xz(rows, *pose)
    ex = pr.exact_stats(x, z, pr.paths(rows, f), rows[:, 7])
    _, _, _, e_w, _, b_rms = pr.sum_bounds(ex)
    f_exact = complex(rr.psf_field_exact(rows, *pose, [pr.F_LOCAL[0]], [pr.F_LOCAL[1]])[0, 0])
    b_st = float(pr.strehl_bound(n, abs(f_exact), pr.field_bound(rows, *pose, *pr.F_LOCAL, f_exact), ex["s"]))
    print("E_row %.3g  B_rms %.3g  E_w %.3g  B_strehl %.3g" % (e_row, float(b_rms), float(e_w), b_st))
    assert st[pr.W_RMS] <= e_row + float(b_rms)
    assert st[pr.W_HI] - st[pr.W_LO] <= 2 * (2 * e_row + float(e_w)) * (1 + 2.0 ** -53)
    assert abs(st[pr.W_MEAN] - pr.FOCUS_R) <= e_row + float(e_w)
    k = st[pr.K_MIN]
    assert 1 - (2 * k * e_row) ** 2 - b_st <= st[pr.STREHL] <= 1 + b_st
    assert b_st < 1e-6
    # the reference point moved sideways by 20 um: 0.75 um of path across the f/13 cone
    moved = (pr.F_LOCAL[0] + 20e-6, pr.F_LOCAL[1])
    st2, _ = abi.psf_stats(rows, *pose, ref=moved)
    _report("moved reference", st2)
    assert st2[pr.STREHL] < 1 and st2[pr.W_RMS] > 1e-7
    assert pr.stat_violations(st2, rows, *pose, ref=moved) == []


@pytest.fixture(scope="module")
def airy_rows():
    system, cs, psfd, lam, D = airy_setup(num_rays=1000)
    bmo.solve_system(system, cs)
    assert len(psfd.data) == 1000
    o = np.asarray(psfd.orientation(), dtype=np.float64)
    return psfd, psfd.data.copy(), (np.asarray(psfd.position(), dtype=np.float64), o[:, 0].copy(), o[:, 2].copy())


def test_field_agrees_with_the_existing_read_out(airy_rows):
    """F is the field of bmo_psf_intensity at the reference point: both are inside psf_engine_bound of the oracle's value."""
    psfd, rows, pose = airy_rows
    for ref in (None, (3e-6, -2e-6)):
        st, _ = abi.psf_stats(rows, *pose, ref=ref)
        _report("airy, ref %s" % (ref,), st)
        _, F, _ = abi.psf_intensity(rows, *pose, [st[pr.X_REF]], [st[pr.Z_REF]], want_field=True)
        err = abs(complex(st[pr.F_RE], st[pr.F_IM]) - F[0, 0])
        print("|F_stats - F_readout| = %.3g (bound %.3g)" % (err, 2 * rr.psf_engine_bound(rows)))
        assert err <= 2 * rr.psf_engine_bound(rows)
        assert pr.stat_violations(st, rows, *pose, ref=ref) == []
        # 0.13 mm inside the paraxial focus of a spherical lens: an aberrated spot
        assert 0 < st[pr.STREHL] < 1
    assert same_bits(psfd.stats(), abi.psf_stats(rows, *pose)[0])


def test_engine_solution_reads_resident_rows(airy_rows):
    """EngineSolution.psf_stats / psf_intensity on a resident result: the single call's statistics, and the sweep read-out with K = 1."""
    psfd, rows, pose = airy_rows
    system, cs, psfd2, lam, D = airy_setup(num_rays=1000)
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    pos, ori = np.asarray(psfd2.position(), dtype=np.float64), np.asarray(psfd2.orientation(), dtype=np.float64)
    for record in (True, False):
        res = eng.trace_device(dev, 100, record_segments=record)
        sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
        try:
            st = sol.psf_stats(0, pos, ori)
            assert same_bits(st, abi.psf_stats(rows, *pose)[0]), record
            ptr, cnt = eng.result_device_hits(res, 0)
            assert same_bits(st, abi.psf_stats(None, *pose, hits_device_ptr=ptr, n_hits=cnt)[0])
            for kw in (dict(), dict(crop_factor=5, center="bbox")):
                xs, zs, I = sol.psf_intensity(0, pos, ori, n=24, **kw)
                ax, az = bmo.components.psf_axes_from_stats(st, n=24, **kw)
                assert np.array_equal(xs, ax) and np.array_equal(zs, az)
                assert np.array_equal(I, abi.psf_intensity(rows, *pose, ax, az)[0]), (record, kw)
        finally:
            sol.handle = None  # the engine frees the result
            eng.free_result(res)
    eng.free_batch(dev)
    eng.close()
