"""Spotdetector read-out on the GPU (bmo_spot_image / bmo_spot_stats and their resident-row forms on an ordinary result): the image equals
the numpy restatement of the binning rule exactly, the statistics lie inside the bounds derived in spot_ref.py from the exact values."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import scenes
import spot_ref as sr

pytestmark = pytest.mark.gpu
mm = 1e-3
WINDOW = (-2.5 * mm, 2.5 * mm, -1.0 * mm, 3.0 * mm)
N_ROWS = [0, 1, 63, 64, 65, 255, 256, 257, 5000]
SHAPES = [(1, 1), (7, 3), (1, 33), (300, 1), (128, 128), (129, 128)]


def _check_image(rows, window, nx, nz, what):
    got, outside, _ = abi.spot_image(rows, window, nx, nz)
    want, want_out = sr.bin_rule(rows, window, nx, nz)
    assert got.shape == (nx, nz) and got.dtype == np.int64, what
    assert outside == want_out, what
    assert np.array_equal(got, want), what
    assert int(got.sum()) + outside == len(rows), what
    return got


@pytest.mark.parametrize("row_cols", [2, 9])
def test_image_equals_the_numpy_rule(row_cols):
    assert 128 * 128 <= sr.LDS_BINS < 129 * 128  # the largest image in LDS and the smallest in global memory
    for n in N_ROWS:
        rows = sr.window_rows(n, WINDOW, seed=100 + n, row_cols=row_cols)
        for nx, nz in SHAPES:
            _check_image(rows, WINDOW, nx, nz, (n, nx, nz, row_cols))


def test_contention():
    nx, nz = 16, 8
    x0, x1, z0, z1 = WINDOW
    cx = lambda i: x0 + (i + 0.5) * (x1 - x0) / nx  # noqa: E731  (bin centres)
    cz = lambda j: z0 + (j + 0.5) * (z1 - z0) / nz  # noqa: E731
    same = np.tile([cx(5), cz(2)], (5000, 1))
    got = _check_image(same, WINDOW, nx, nz, "identical rows")
    assert got[5, 2] == 5000
    two = np.array([[cx(3 + 9 * (k % 2)), cz(1 + 4 * (k % 2))] for k in range(64)])
    got = _check_image(two, WINDOW, nx, nz, "two bins")
    assert got[3, 1] == 32 and got[12, 5] == 32
    runs = np.array([[cx((k // 3) % nx), cz((k // 3) // nx % nz)] for k in range(257)])
    _check_image(runs, WINDOW, nx, nz, "runs of three")
    # the same three through the global-memory path
    for rows in (same, two, runs):
        _check_image(rows, WINDOW, 129, 128, "global path")


def test_split_boundary_inside_one_call():
    n = sr.smallest_ragged_three_splits()
    ns, per = sr.spot_splits(n)
    assert ns >= 3 and n % per != 0
    rows = sr.window_rows(n, WINDOW, seed=7)
    for nx, nz in ((7, 3), (129, 128)):
        _check_image(rows, WINDOW, nx, nz, (n, nx, nz))
    fin = sr.finite_rows(n, seed=8)
    st, _ = abi.spot_stats(fin)
    assert sr.stat_violations(st, fin) == []


@pytest.fixture(scope="module")
def c2_solutions():
    """The config-2 scene solved on 4096 rays, and on the two contiguous halves of that bundle: (scene, [(TraceResult, EngineSolution)] x 3)."""
    system, _ = scenes.c2_scene()
    bundle = scenes.c2_bundle(4096)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    parts = [bundle] + [bmo.RayBundle(bundle.kind, np.ascontiguousarray(bundle.planes[:, a:b])) for a, b in ((0, 2048), (2048, 4096))]
    sols = [bmo.system._engine_solve(scene, p, 100, None) for p in parts]
    yield scene, sols
    for _, sol in sols:
        sol.free()


def _packed_columns(sol, slot, n):
    buf = np.zeros((n, 2))
    abi.check(sol.lib, sol.lib.bmo_result_copy_hit_columns(sol.handle, slot, 2, buf.ctypes.data_as(C.c_void_p), n), "bmo_result_copy_hit_columns")
    return buf


def test_resident_rows_equal_host_rows(c2_solutions):
    scene, sols = c2_solutions
    res, sol = sols[0]
    window = (-2.5 * mm, 2.5 * mm, -2.5 * mm, 2.5 * mm)
    seen = 0
    for slot, det in enumerate(scene.detectors):
        assert isinstance(det, bmo.Spotdetector)
        n = int(res.det_count[slot])
        rows = _packed_columns(sol, slot, n)
        assert np.array_equal(rows, res.detector_hits(slot)[:, 0:2])
        seen += n
        for nx, nz in ((64, 48), (129, 128)):
            img, outside = sol.spot_image(slot, window, nx, nz)
            img_h, outside_h, _ = abi.spot_image(rows, window, nx, nz)
            want, want_out = sr.bin_rule(rows, window, nx, nz)
            assert np.array_equal(img, img_h) and np.array_equal(img, want)
            assert outside == outside_h == want_out and int(img.sum()) + outside == n
        st = sol.spot_stats(slot)
        st_h, _ = abi.spot_stats(rows)
        assert st.tobytes() == st_h.tobytes()
        assert sr.stat_violations(st, rows) == []
        assert sol.readout_ms > 0
    assert seen > 4096  # both arms of the splitter recorded


@pytest.mark.parametrize("n", N_ROWS)
def test_statistics_within_derived_bounds(n):
    for cols, seed in ((2, 31), (9, 32)):
        rows = sr.finite_rows(n, seed + n, row_cols=cols)
        st, _ = abi.spot_stats(rows)
        assert sr.stat_violations(st, rows) == [], (n, cols)
        if n == 0:
            assert st[sr.N] == 0 and np.isnan(st[1:]).all()
        if n == 1:
            assert st[sr.N] == 1 and st[sr.CX] == rows[0, 0] and st[sr.CZ] == rows[0, 1]
            assert not st[sr.MXX:].any() and not np.signbit(st[sr.MXX:]).any()
        if n > 0:  # exact: count and extrema
            assert st[sr.N] == n
            assert (st[sr.X_MIN], st[sr.X_MAX], st[sr.Z_MIN], st[sr.Z_MAX]) == (rows[:, 0].min(), rows[:, 0].max(), rows[:, 1].min(), rows[:, 1].max())


def test_statistics_of_the_offset_spot():
    rows = sr.offset_spot()
    st, _ = abi.spot_stats(rows)
    bad = sr.stat_violations(st, rows)
    assert bad == [], bad


def test_shards_add_to_the_whole_bundle(c2_solutions):
    scene, sols = c2_solutions
    window = (-1.0 * mm, 1.5 * mm, -2.0 * mm, 2.5 * mm)
    for slot in range(len(scene.detectors)):
        whole, lo, hi = (sol.spot_image(slot, window, 96, 80) for _, sol in sols)
        assert sols[1][0].det_count[slot] + sols[2][0].det_count[slot] == sols[0][0].det_count[slot] > 0
        assert np.array_equal(lo[0] + hi[0], whole[0]) and lo[1] + hi[1] == whole[1]
        assert whole[0].sum() > 0


def _sweep_rcs(handle, slot, K):
    """Return codes of the two resident-row entries on a K-configuration request."""
    lib = abi.load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    K1 = max(K, 1)
    w = np.tile([-1e-3, 1e-3, -1e-3, 1e-3], (K1, 1))
    img, out, st = np.zeros(K1 * 16, dtype=np.int64), np.zeros(K1, dtype=np.int64), np.zeros(K1 * 12)
    return (lib.bmo_spot_image_sweep(handle, slot, K, w.ctypes.data_as(dp), 4, 4, img.ctypes.data_as(ip), out.ctypes.data_as(ip), None),
            lib.bmo_spot_stats_sweep(handle, slot, K, st.ctypes.data_as(dp), None))


def test_refusals_that_need_a_result(c2_solutions):
    INVALID, UNSUPPORTED = -1, -4
    scene, sols = c2_solutions
    _, sol = sols[0]
    assert _sweep_rcs(sol.handle, 0, 1) == (0, 0)
    for slot in (-1, len(scene.detectors), 99):
        assert _sweep_rcs(sol.handle, slot, 1) == (INVALID, INVALID), slot
    for K in (0, 2):
        assert _sweep_rcs(sol.handle, 0, K) == (INVALID, INVALID), K  # an ordinary result has one configuration
    # slots of the other two detector kinds, in a Ray solution
    psfd, pd, spot = bmo.PSFDetector(5 * mm), bmo.Photodetector(5 * mm, 8), bmo.Spotdetector(5 * mm)
    for k, d in enumerate((psfd, pd, spot)):
        bmo.translate3d(d, [10 * mm * (k - 1), 50 * mm, 0])
    system = bmo.System([psfd, pd, spot])
    bundle = scenes.disc_bundle(64, center=[0, 0, 0], direction=[0, 1, 0], diameter=30 * mm, lam=1e-6, jitter=0.0)
    sc = bmo.CompiledScene(system, bundle.lambdas)
    res2, sol2 = bmo.system._engine_solve(sc, bundle, 100, None)
    try:
        kinds = {type(d): slot for slot, d in enumerate(sc.detectors)}
        assert _sweep_rcs(sol2.handle, kinds[bmo.PSFDetector], 1) == (INVALID, INVALID)
        assert b"Spotdetector" in abi.load_engine().bmo_last_error()
        assert _sweep_rcs(sol2.handle, kinds[bmo.Photodetector], 1) == (INVALID, INVALID)
        assert _sweep_rcs(sol2.handle, kinds[bmo.Spotdetector], 1) == (0, 0)
    finally:
        sol2.free()
    # a GaussianBeamlet solution: three rows per beamlet in the slot, no Spotdetector method in the reference
    system3, _ = scenes.c2_scene()
    b3 = scenes.c3_bundle(64)
    sc3 = bmo.CompiledScene(system3, b3.lambdas)
    res3, sol3 = bmo.system._engine_solve(sc3, b3, 100, None)
    try:
        assert _sweep_rcs(sol3.handle, 0, 1) == (UNSUPPORTED, UNSUPPORTED)
        with pytest.raises(RuntimeError, match="bmo_spot_stats_sweep"):
            sol3.spot_stats(0)
    finally:
        sol3.free()


def test_spotdetector_methods_read_the_accumulated_rows():
    lens = bmo.SphericalLens(100 * mm, float("inf"), 1 * mm, 25.4 * mm, lambda lam_: 1.5)
    sd = bmo.Spotdetector(4 * mm)
    bmo.translate3d(sd, [0, 150 * mm, 0])
    system = bmo.System([lens, sd])
    with pytest.raises(ValueError, match="no row"):
        sd.image(8, window="extent")
    counts = []
    for num_rays, dia in ((300, 8 * mm), (500, 14 * mm)):  # 2 mm and 3.5 mm across on the 4 mm detector, 50 mm before the focus
        cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], dia, 1e-6, num_rays=num_rays)
        bmo.solve_system(system, cs)
        counts.append(len(sd.data))
    assert counts == [300, 800]
    xe, ze, img, outside = sd.image(32, 20)
    assert xe.shape == (33,) and ze.shape == (21,) and (xe[0], xe[-1], ze[0], ze[-1]) == (-2 * mm, 2 * mm, -2 * mm, 2 * mm)
    want, want_out = sr.bin_rule(sd.data, (-2 * mm, 2 * mm, -2 * mm, 2 * mm), 32, 20)
    assert np.array_equal(img, want) and outside == want_out and int(img.sum()) + outside == 800
    st = sd.stats()
    assert st[sr.N] == 800 and sr.stat_violations(st, sd.data) == []
    xe, ze, img, outside = sd.image(16, window="extent")
    assert (xe[0], xe[-1], ze[0], ze[-1]) == tuple(st[sr.X_MIN:sr.Z_MAX + 1]) and outside == 0 and img.sum() == 800 and img.shape == (16, 16)
    bmo.release(cs)
    # rows that share one x have no extent to bin on
    line = bmo.Spotdetector(4 * mm)
    line.data = np.array([[0.5 * mm, -1 * mm], [0.5 * mm, 1 * mm], [0.5 * mm, 0.25 * mm]])
    with pytest.raises(ValueError, match="zero extent"):
        line.image(8, window="extent")
    assert line.image(8)[2].sum() == 3  # the face still works
