"""Through-focus read-out on the GPU: bmo_psf_through_focus against the 40-digit stack and against bmo_psf_intensity at the displaced origin,
bmo_psf_focus_stats against the 40-digit propagated statistics and against bmo_psf_stats, and both against a second solve with the detector
moved, which is what the reference does.  Every bound is derived in tests/focus_ref.py; nothing is fitted."""
import math

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import focus_ref as fr
import psf_stats_ref as pr
import readout_ref as rr
import spot_ref as sr

pytestmark = pytest.mark.gpu

MP = fr.source_focus_mp()
mm = 1e-3


def _solve(num_rays, move_along_y=0.0, record=True, keep=False):
    """tilted_psf_case solved on the GPU with the detector moved by `move_along_y` along its local y: (rows, (pos, e1, e2), orientation)."""
    system, psfd, bundle = rr.tilted_psf_case(num_rays)
    if move_along_y:
        bmo.translate3d(psfd, list(move_along_y * np.asarray(psfd.orientation(), dtype=np.float64)[:, 1]))
    scene = bmo.CompiledScene(system, bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    dev = eng.upload(bundle)
    res = eng.trace_device(dev, 100, record_segments=record)
    rows = eng.result_view(res).detector_hits(0).copy()
    assert len(rows) == num_rays  # the whole oblique bundle lands on the detector
    pos, o = np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)
    if keep:
        return rows, (pos, o[:, 0].copy(), o[:, 2].copy()), o, (eng, dev, res, bundle)
    eng.free_result(res)
    eng.free_batch(dev)
    eng.close()
    return rows, (pos, o[:, 0].copy(), o[:, 2].copy()), o


@pytest.fixture(scope="module")
def case600():
    rows, pose, o = _solve(600)
    assert np.all(np.abs(pose[1]) > 1e-3) and np.all(np.abs(pose[2]) > 1e-3) and (rows[:, 3:6] != 0).all()
    return rows, pose, o


@pytest.fixture(scope="module")
def moved300():
    """The detector at its place and moved by +0.3 mm and -0.2 mm along its local y, 300 rays each: (rows, pose, {offset: (rows, pose)})."""
    rows, pose, o = _solve(300)
    return rows, pose, o, {off: _solve(300, off)[:2] for off in (0.3 * mm, -0.2 * mm)}


def _axes(rows, pose, o, n):
    return bmo.components.psf_sample_axes(rows, pose[0], o, n=n, crop_factor=5, center="bbox")


def _oblique(pose, M):
    """M displacements up to +-0.5 mm along the normal with a lateral part, no zero component"""
    origin, e1, e2 = pose
    t = -0.5 * mm + 1.0 * mm * (np.arange(M) + 0.37) / M
    d = t[:, None] * (np.cross(e1, e2) + 0.05 * e1 - 0.03 * e2)[None, :]
    assert (d != 0).all() and np.abs(d).max() <= 0.5 * mm
    return d


def _inside(got, want, bound, what):
    err = max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    print("%s: largest component error %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def test_stack_against_the_exact_field(case600):
    """H = 600: three splits of one LDS tile each, the last ragged (88 rows); n = 5: one partial point block; M = MP + 1 crosses the chunk."""
    rows, pose, o = case600
    n, M = 5, MP + 1
    assert rr.source_psf_tile() == rr.PSF_TILE and rr.psf_tiles(600, n * n) == [[256], [256], [88]]
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    I, F, ms = abi.psf_through_focus(rows, *pose, d, xs, zs, want_field=True)
    assert I.shape == F.shape == (M, n, n) and ms > 0
    assert np.array_equal(I, F.real * F.real + F.imag * F.imag)  # abs2 of the field it returns
    planes, sub = [0, MP - 1, MP], [0, 2, 4]
    exact = fr.through_focus_exact(rows, *pose, d[planes], xs[sub], zs[sub])
    for q, m in enumerate(planes):
        bound = fr.stack_bound(rows, *pose, d[m], xs[sub], zs[sub], f_abs=np.abs(exact[q]).max())
        _inside(F[m][np.ix_(sub, sub)], exact[q], bound, "plane %d" % m)
        assert bound < 2e-9 * rows[:, 7].sum()  # the bound has teeth: the planes differ among themselves by far more
    assert np.abs(F[0] - F[MP]).max() > 1e-6 * rows[:, 7].sum()


def test_stack_against_the_direct_path(case600):
    """n = 17: 289 points, the second point block is partial.  Every plane against bmo_psf_intensity at the double origin + d_m: both are
    inside their bounds of the exact field at the exact origin + d_m, the direct path's point being off it by the rounding of the origin.
    The plane with d = 0 has the factor (1, 0) and the same split plan: bit for bit."""
    rows, pose, o = case600
    n, M, zero = 17, MP + 1, 3
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    d[zero] = 0.0
    I, F, _ = abi.psf_through_focus(rows, *pose, d, xs, zs, want_field=True)
    for m in range(M):
        moved = pose[0] + d[m]
        I_d, F_d, _ = abi.psf_intensity(rows, moved, pose[1], pose[2], xs, zs, want_field=True)
        f_abs = np.abs(F_d).max() * (1 + 1e-6)
        bound = (fr.stack_bound(rows, *pose, d[m], xs, zs, f_abs) + fr.intensity_bound(rows, moved, pose[1], pose[2], xs, zs, f_abs)
                 + fr.origin_shift_term(rows, pose[0], d[m], moved))
        _inside(F[m], F_d, bound, "plane %d" % m)
        assert np.abs(I[m] - I_d).max() <= 2 * f_abs * math.sqrt(2) * bound * (1 + 1e-6) + 8 * fr.U * f_abs ** 2
        if m == zero:
            assert np.array_equal(I[m].view(np.uint64), I_d.view(np.uint64)) and np.array_equal(F[m], F_d)


@pytest.mark.parametrize("H,M", [(0, 3), (1, 3), (256, MP + 1), (600, 1), (600, 2), (600, 3), (600, 6), (600, 11), (600, MP), (600, 2 * MP + 5)])
def test_edge_shapes(case600, H, M):
    """No rows, one row, exactly one tile; and every kernel the stack launches: full chunks of MP planes, and for the planes that are left
    the kernel of 1, 2, 4, 8 or 16 slots (M = 1, 2, 3, 6, 11; M = MP + 1 and 2 MP + 5 have both).  Every plane against the direct path inside
    the derived bounds; the last plane, which the remainder kernel computes, has d = 0 and equals bmo_psf_intensity bit for bit."""
    rows, pose, o = case600
    n = 5
    xs, zs = _axes(rows, pose, o, n)
    d = _oblique(pose, M)
    d[M - 1] = 0.0
    I, F, _ = abi.psf_through_focus(rows[:H], *pose, d, xs, zs, want_field=True)
    assert I.shape == (M, n, n)
    if H == 0:
        assert not I.any() and not F.any()
        return
    for m in range(M):
        moved = pose[0] + d[m]
        I_d, F_d, _ = abi.psf_intensity(rows[:H], moved, pose[1], pose[2], xs, zs, want_field=True)
        f_abs = np.abs(F_d).max() * (1 + 1e-6)
        bound = (fr.stack_bound(rows[:H], *pose, d[m], xs, zs, f_abs) + fr.intensity_bound(rows[:H], moved, pose[1], pose[2], xs, zs, f_abs)
                 + fr.origin_shift_term(rows[:H], pose[0], d[m], moved))
        _inside(F[m], F_d, bound, "H = %d, plane %d" % (H, m))
        assert np.array_equal(I[m], F[m].real * F[m].real + F[m].imag * F[m].imag)
        if m == M - 1:
            assert np.array_equal(I[m].view(np.uint64), I_d.view(np.uint64)) and np.array_equal(F[m], F_d)


def test_a_stack_of_two_passes(case600):
    """A stack whose partial sums pass 1 GiB runs in passes of whole chunks: 2^19 rows on n = 17 make 2 048 splits, 9.5 MB of partial sums
    per plane, 112 planes per pass; M = 128 is a pass of 112 planes and one of 16.  The planes at the ends of both passes against the direct
    path on the same resident rows; plane 112, the first of the second pass, has d = 0 and equals it bit for bit.  The rows are the 600
    traced ones repeated, so the bounds' geometry (the largest phase and |p - hit|_1, both attained at the corners of the grid: the phase is
    linear in (x, z), the 1-norm convex) is that of the 600."""
    import ctypes as C

    rows600, pose, o = case600
    n, M, H = 17, 128, 1 << 19
    rows = np.ascontiguousarray(np.tile(rows600, (H // 600 + 1, 1))[:H])
    ns, per = rr.psf_splits(H, n * n)
    per_plane = ns * n * n * 16
    per_pass = (1 << 30) // per_plane // MP * MP
    assert ns == 2048 and 0 < per_pass < M <= 2 * per_pass and per_pass == 112
    xs, zs = _axes(rows600, pose, o, n)
    d = _oblique(pose, M)
    d[per_pass] = 0.0
    hip = C.CDLL("libamdhip64.so")
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(rows.nbytes)) == 0
    try:
        assert hip.hipMemcpy(dptr, C.c_void_p(rows.ctypes.data), C.c_size_t(rows.nbytes), 1) == 0  # hipMemcpyHostToDevice
        kw = dict(hits_device_ptr=dptr.value, n_hits=H, want_field=True)
        I, F, ms = abi.psf_through_focus(None, *pose, d, xs, zs, **kw)
        assert I.shape == (M, n, n) and ms > 0
        corners = [0, n - 1]
        scale = H / 600 + 1  # sum proj and the row count of the bound, against those of the 600 rows it is evaluated on
        for m in (0, per_pass - 1, per_pass, per_pass + 1, M - 1):
            moved = pose[0] + d[m]
            I_d, F_d, _ = abi.psf_intensity(None, moved, pose[1], pose[2], xs, zs, **kw)
            f_abs = np.abs(F_d).max() * (1 + 1e-6)
            args = (fr.arg_point(rows600, *pose, xs[corners], zs[corners]) + fr.arg_point(rows600, moved, pose[1], pose[2], xs[corners], zs[corners])
                    + 4 * fr.U * float(rows[:, 8].max()) * float(np.abs(d[m]).sum()))
            bound = ((args + (fr.C_TERM + fr.C_TERM_DIRECT) * fr.U + 2 * (H + 1) * fr.U) * float(rows[:, 7].sum()) * (1 + 1e-9) + 2 * fr.U * f_abs
                     + scale * fr.origin_shift_term(rows600, pose[0], d[m], moved))
            _inside(F[m], F_d, bound, "two passes, plane %d" % m)
            assert np.array_equal(I[m], F[m].real * F[m].real + F[m].imag * F[m].imag)
            if m == per_pass:
                assert np.array_equal(I[m].view(np.uint64), I_d.view(np.uint64)) and np.array_equal(F[m], F_d)
    finally:
        hip.hipFree(dptr)


def test_resident_rows_are_refused_where_they_are_not_psf_rows():
    """EngineSolution.psf_focus_stats / psf_through_focus ask the library for the rows (bmo_result_psf_rows): a slot of another detector
    kind is BMO_ERR_INVALID, a GaussianBeamlet solution BMO_ERR_UNSUPPORTED."""
    import scenes

    psfd, spot = bmo.PSFDetector(5 * mm), bmo.Spotdetector(5 * mm)
    bmo.translate3d(psfd, [-5 * mm, 50 * mm, 0])
    bmo.translate3d(spot, [5 * mm, 50 * mm, 0])
    bundle = scenes.disc_bundle(64, center=[0, 0, 0], direction=[0, 1, 0], diameter=18 * mm, lam=1e-6, jitter=0.0)
    sc = bmo.CompiledScene(bmo.System([psfd, spot]), bundle.lambdas)
    _, sol = bmo.system._engine_solve(sc, bundle, 100, None)
    try:
        kinds = {type(dd): slot for slot, dd in enumerate(sc.detectors)}
        pos, ori = np.asarray(psfd.position(), dtype=np.float64), np.asarray(psfd.orientation(), dtype=np.float64)
        st = sol.psf_focus_stats(kinds[bmo.PSFDetector], pos, ori, [0.0, 1e-4])
        assert st.shape == (2, 12) and st[0, fr.N] > 0
        for slot in (kinds[bmo.Spotdetector], -1, 2):
            with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-1\)"):
                sol.psf_focus_stats(slot, pos, ori, [0.0])
            with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-1\)"):
                sol.psf_through_focus(slot, pos, ori, [0.0], n=4)
    finally:
        sol.free()
    system3, _ = scenes.c2_scene()
    b3 = scenes.c3_bundle(64)
    _, sol3 = bmo.system._engine_solve(bmo.CompiledScene(system3, b3.lambdas), b3, 100, None)
    try:
        with pytest.raises(RuntimeError, match=r"bmo_result_psf_rows failed \(-4\).*GaussianBeamlet"):
            sol3.psf_through_focus(0, np.zeros(3), np.eye(3), [0.0], n=4)
    finally:
        sol3.free()


def test_resident_rows_and_the_python_mirror():
    """After a detector-only solve EngineSolution reads the resident rows: bit for bit what PSFDetector.through_focus reads from the copied
    rows; follow="centroid" centres every plane on its own centroid, follow=None on the window plane's."""
    rows, pose, o, (eng, dev, res, bundle) = _solve(600, record=False, keep=True)
    sol = bmo.system.EngineSolution(eng.lib, res, bundle.n, bundle.kind)
    psfd = bmo.PSFDetector(10 * mm)
    psfd.data, psfd.position, psfd.orientation = rows, (lambda: pose[0]), (lambda: o)
    offsets = np.linspace(-0.4 * mm, 0.4 * mm, 5)
    try:
        st = sol.psf_focus_stats(0, pose[0], o, offsets)
        assert np.array_equal(st, psfd.focus_stats(offsets)) and np.isfinite(st).all() and sol.readout_ms > 0
        assert np.array_equal(st, abi.psf_focus_stats(rows, *pose, o[:, 1], offsets)[0])
        for kw in (dict(), dict(follow=None, window_plane=1, crop_factor=3), dict(axis=np.cross(pose[1], pose[2]))):
            got, want = sol.psf_through_focus(0, pose[0], o, offsets, n=9, **kw), psfd.through_focus(offsets, n=9, **kw)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), kw
            xs, zs, d, I, st_k = got
            axis = kw.get("axis", o[:, 1])
            w = kw.get("window_plane", int(np.argmin(st_k[:, fr.RMS_R])))
            centre = st_k[:, [fr.CX, fr.CZ]] if kw.get("follow", "centroid") == "centroid" else np.tile(st_k[w, [fr.CX, fr.CZ]], (5, 1))
            assert np.array_equal(d, offsets[:, None] * axis[None, :] + centre[:, 0:1] * pose[1][None, :] + centre[:, 1:2] * pose[2][None, :])
            hw = st_k[w, [fr.HWX, fr.HWZ]] * kw.get("crop_factor", 1)
            assert xs[0] == -hw[0] and xs[-1] == hw[0] and zs[0] == -hw[1] and zs[-1] == hw[1] and I.shape == (5, 9, 9)
            assert np.array_equal(I, abi.psf_through_focus(rows, *pose, d, xs, zs)[0])
        t, r = bmo.components.best_focus(offsets, st[:, fr.RMS_R])
        assert offsets[0] <= t <= offsets[-1] and 0 < r <= st[:, fr.RMS_R].min()
    finally:
        sol.handle = None  # the engine frees the result
        eng.free_result(res)
        eng.free_batch(dev)
        eng.close()


def test_a_second_solve_with_the_detector_moved(moved300):
    """What the reference does for another plane: translate the PSFDetector along its local y, solve again, read intensity(psf) there.  The
    through-focus plane of the FIRST solve's rows, at the displacement between the two detector positions and on the same axes, agrees inside
    the two engine bounds plus k S times the path discrepancy between the two solves' rows, which is evaluated in mpmath from the rows
    themselves (focus_ref.row_discrepancy) and must stay below 1e-12 m.  Measured: 2.28e-16 m (+0.3 mm) and 2.07e-16 m (-0.2 mm), on the CPU
    oracle's rows and on the GPU's alike; the field then differs by 5e-9 against a bound of 7.5e-7 (sum proj = 300)."""
    rows, pose, o, moved = moved300
    n = 9
    for off, (rows_b, pose_b) in moved.items():
        assert np.array_equal(pose_b[1], pose[1]) and np.array_equal(pose_b[2], pose[2])
        d = pose_b[0] - pose[0]
        assert abs(np.dot(d, o[:, 1]) - off) < 1e-15
        xs, zs = _axes(rows_b, pose_b, o, n)
        I_b, F_b, _ = abi.psf_intensity(rows_b, *pose_b, xs, zs, want_field=True)
        I, F, _ = abi.psf_through_focus(rows, *pose, [d], xs, zs, want_field=True)
        disc, _ = fr.row_discrepancy(rows, rows_b, pose_b[0], pose[1], pose[2], np.zeros(3))
        print("offset %+.1e m: path discrepancy of the rows %.3e m" % (off, disc))
        assert disc < 1e-12
        f_abs = np.abs(F_b).max() * (1 + 1e-6)
        k_s = float(rows[:, 8].max()) * float(rows[:, 7].sum())
        bound = (fr.stack_bound(rows, *pose, d, xs, zs, f_abs) + fr.intensity_bound(rows_b, *pose_b, xs, zs, f_abs)
                 + fr.origin_shift_term(rows, pose[0], d, pose_b[0]) + k_s * disc)
        _inside(F[0], F_b, bound, "offset %+.1e" % off)
        assert np.abs(I[0] - I_b).max() <= 2 * f_abs * math.sqrt(2) * bound * (1 + 1e-6) + 8 * fr.U * f_abs ** 2
        assert np.abs(F_b - abi.psf_intensity(rows, *pose, xs, zs, want_field=True)[1]).max() > 1e3 * bound  # the plane did move


# ------------------------------------------------------------------------------------------------ the statistics
H_STATS = 2100


@pytest.fixture(scope="module")
def case2100():
    ns, per = sr.spot_splits(H_STATS)
    assert ns == 2 and H_STATS > per and (H_STATS - per) % 256 != 0  # two splits, the second ends in a ragged tile
    return _solve(H_STATS)


def test_focus_statistics_against_the_exact_ones(case2100):
    """M = 70 (nine chunks of planes, the last ragged) and M = 3; the planes at the chunk boundary and the ends against the 40-digit
    statistics, the planes the two calls share bit for bit (the order of the sums depends on the row count only), and the plane at offset 0
    against bmo_psf_stats, whose x and z are those of the hits themselves: the hits lie off the plane by at most s_max, which is evaluated."""
    rows, pose, o = case2100
    smp = fr.source_focus_stat_mp()
    axis = o[:, 1]
    off70 = np.linspace(-0.5 * mm, 0.5 * mm, 70)
    off70[smp] = 0.0
    shared = [0, smp, 69]
    st70, ms = abi.psf_focus_stats(rows, *pose, axis, off70)
    st3, _ = abi.psf_focus_stats(rows, *pose, axis, off70[shared])
    assert st70.shape == (70, 12) and st3.shape == (3, 12) and ms > 0 and np.isfinite(st70).all()
    assert np.array_equal(st70[shared].view(np.uint64), st3.view(np.uint64))
    checked = [0, smp - 1, smp, 69]
    exact = fr.focus_stats_exact(rows, *pose, axis, off70[checked])
    for m, ex in zip(checked, exact):
        bad = fr.stat_violations(st70[m], ex)
        print("plane %d (offset %+.3e): RMS_R %.6e  bounds CX %.2e RMS_R %.2e" % (m, off70[m], st70[m, fr.RMS_R], fr.stat_bounds(ex)[fr.CX], fr.stat_bounds(ex)[fr.RMS_R]))
        assert bad == [], (m, bad)
    assert abs(st70[0, fr.RMS_R] - st70[69, fr.RMS_R]) > 1e6 * fr.stat_bounds(exact[0])[fr.RMS_R]  # the planes differ by far more than a bound
    # offset 0 against bmo_psf_stats
    ex0, b0 = exact[2], fr.stat_bounds(exact[2])
    ps = abi.psf_stats(rows, *pose)[0]
    x, z = pr.local_xz(rows, *pose)
    _, e_cx, e_cz, _, _, _ = pr.sum_bounds(pr.exact_stats(x, z, pr.paths(rows, pose[0]), rows[:, 7]))
    print("offset 0: the hits lie within %.2e m of the plane" % ex0["s_max"])
    assert ex0["s_max"] < 1e-12  # otherwise the two statistics are of different points and the comparison below would only widen
    for col_f, col_p, e_p in ((fr.CX, pr.CX, float(e_cx)), (fr.CZ, pr.CZ, float(e_cz))):
        assert abs(st70[smp, col_f] - ps[col_p]) <= b0[col_f] + e_p + ex0["s_max"]
    for col_f, col_p, e_p in ((fr.HWX, pr.HWX, float(e_cx)), (fr.HWZ, pr.HWZ, float(e_cz))):
        assert abs(st70[smp, col_f] - ps[col_p]) <= b0[col_f] + (e_p + fr.U * ps[col_p]) * (1 + 1e-9) + 2 * ex0["s_max"]


def test_focus_statistics_against_a_second_solve(moved300):
    """bmo_psf_stats of the moved detector's own rows against the focus statistics of the first solve's rows at that offset: centroids and
    half-widths inside both bounds plus the position discrepancy of the rows, evaluated in mpmath, and the rounding of the moved origin."""
    rows, pose, o, moved = moved300
    offs = list(moved)
    st, _ = abi.psf_focus_stats(rows, *pose, o[:, 1], offs)
    exact = fr.focus_stats_exact(rows, *pose, o[:, 1], offs)
    for m, off in enumerate(offs):
        rows_b, pose_b = moved[off]
        assert fr.stat_violations(st[m], exact[m]) == []
        b = fr.stat_bounds(exact[m])
        ps = abi.psf_stats(rows_b, *pose_b)[0]
        x, z = pr.local_xz(rows_b, *pose_b)
        _, e_cx, e_cz, _, _, _ = pr.sum_bounds(pr.exact_stats(x, z, pr.paths(rows_b, pose_b[0]), rows_b[:, 7]))
        _, pos_disc = fr.row_discrepancy(rows, rows_b, pose_b[0], pose[1], pose[2], np.zeros(3))
        slack = pos_disc + fr.origin_offset(pose[0], off * o[:, 1], pose_b[0]) + 3 * fr.U * np.abs(off * o[:, 1]).sum()  # off * axis in doubles
        print("offset %+.1e m: position discrepancy of the rows %.3e m, of the origins %.3e m" % (off, pos_disc, slack - pos_disc))
        assert pos_disc < 1e-12 and slack < 1e-12
        for col_f, col_p, e_p in ((fr.CX, pr.CX, float(e_cx)), (fr.CZ, pr.CZ, float(e_cz))):
            assert abs(st[m, col_f] - ps[col_p]) <= b[col_f] + e_p + slack, (off, col_f)
        for col_f, col_p, e_p in ((fr.HWX, pr.HWX, float(e_cx)), (fr.HWZ, pr.HWZ, float(e_cz))):
            assert abs(st[m, col_f] - ps[col_p]) <= b[col_f] + (e_p + fr.U * ps[col_p]) * (1 + 1e-9) + 2 * slack, (off, col_f)


def test_rows_without_statistics_do_not_fault(case600):
    """No rows: N = 0 and NaN; a row parallel to the planes (dot(dir, nrm) = 0): N and NaN in every plane, and the call returns."""
    rows, pose, o = case600
    st, _ = abi.psf_focus_stats(rows[:0], *pose, o[:, 1], [0.0, 1e-4])
    assert (st[:, fr.N] == 0).all() and np.isnan(st[:, 1:]).all()
    flat = rows[:300].copy()
    flat[7, 3:6] = [1.0, 0.0, 0.0]
    frame = (pose[0], np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0]))  # nrm = (0, -1, 0): row 7 runs in the plane
    st, _ = abi.psf_focus_stats(flat, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4, -1e-4])
    assert (st[:, fr.N] == 300).all() and np.isnan(st[:, 1:]).all()
    flat[7] = rows[7]
    st, _ = abi.psf_focus_stats(flat, *frame, [0.0, 1.0, 0.0], [0.0, 1e-4, -1e-4])
    assert np.isfinite(st).all()


def test_a_nan_proj_reads_nan_not_what_the_buffer_held(case600):
    """A NaN proj makes S NaN without a row parallel to the planes: S, the centroid and the four spreads about it read NaN, N and the extrema
    are those of the rows.  The call before leaves finite statistics of the same shape behind, which the spread columns must not repeat."""
    rows, pose, o = case600
    offs = [0.0, 1e-4, -1e-4]
    good, _ = abi.psf_focus_stats(rows[:300], *pose, o[:, 1], offs)
    assert np.isfinite(good).all()
    bad = rows[:300].copy()
    bad[7, 7] = np.nan
    st, _ = abi.psf_focus_stats(bad, *pose, o[:, 1], offs)
    nan_cols = [fr.S, fr.CX, fr.CZ, fr.HWX, fr.HWZ, fr.RMS_R, fr.MAX_R]
    kept = [fr.N, fr.X_MIN, fr.X_MAX, fr.Z_MIN, fr.Z_MAX]
    assert np.isnan(st[:, nan_cols]).all() and np.array_equal(st[:, kept], good[:, kept])
