"""Focus statistics and through-focus stacks of sweeps on the GPU (include/bmo_sweep_readout.h): bmo_psf_focus_stats_sweep and
bmo_psf_through_focus_sweep equal, configuration by configuration and bit for bit in every output, bmo_psf_focus_stats and
bmo_psf_through_focus on that configuration's rows with its pose, planes and axes; SweepSolution.psf_focus_stats / psf_best_focus /
psf_through_focus equal components.psf_through_focus driven by single calls on the host rows.

The scenes are those of test_psf_stats_sweep_gpu.py (K = 1, 3, 8: ragged counts, one configuration without rows, a pose per configuration)
and one more three-configuration sweep whose fullest configuration has two row splits with a ragged last tile.  Shapes: M = 1, 9, 17 planes
(9 crosses the 8-plane chunks of the statistics, 17 is a 16-chunk and one slot of the stack), n = 5 and 17 (one partial point block, two)."""
import ctypes as C

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
from bmo_amd import components as cp
import focus_ref as fr
import readout_ref as rr
import spot_ref as sr
from test_psf_readout import airy_setup
from test_psf_stats import same_bits
from test_psf_stats_sweep_gpu import PLACES, RAYS, _pose, _sweep

pytestmark = pytest.mark.gpu
mm = 1e-3
PLANES = (1, 9, 17)
GRIDS = (5, 17)
BIG_RAYS = 2100  # two row splits of 1 280 and 820 rows: the last tile has 52
BIG_PLACES = [(0.0, 200.13 * mm), (3.5 * mm, 120 * mm), (0.0, 199.6 * mm)]


def make_sweep(key, record_segments=True):
    """_sweep(K) of test_psf_stats_sweep_gpu.py for K = 1, 3, 8; "big": three configurations of 2 100 rays, turned like those"""
    if key != "big":
        return _sweep(key, record_segments=record_segments)
    system, cs, psfd, lam, D = airy_setup(num_rays=BIG_RAYS)

    def configure(c):
        x, y = BIG_PLACES[c]
        bmo.translate_to3d(psfd, [x, y, 0.0])
        if c > 0:
            bmo.yrotate3d(psfd, np.radians(7))
            bmo.xrotate3d(psfd, np.radians(0.4))

    return bmo.solve_sweep(system, cs, 3, configure, record_segments=record_segments), psfd


@pytest.fixture(scope="module", params=[1, 3, 8, "big"])
def swept(request):
    key = request.param
    sol, psfd = make_sweep(key)
    rows = [sol.detector_hits(psfd, c).copy() for c in range(sol.n)]
    yield key, sol, psfd, rows
    sol.close()


def poses(sol, psfd):
    """(slot, pos [K, 3], e1s [K, 3], e2s [K, 3], local y [K, 3])"""
    slot = sol._slot(psfd)
    pos = np.ascontiguousarray([sol._poses[c][slot][0] for c in range(sol.n)], dtype=np.float64)
    ori = np.ascontiguousarray([sol._poses[c][slot][1] for c in range(sol.n)], dtype=np.float64)
    return slot, pos, np.ascontiguousarray(ori[:, :, 0]), np.ascontiguousarray(ori[:, :, 2]), np.ascontiguousarray(ori[:, :, 1])


def planes(sol, psfd, rows, M, seed=0):
    """Planes of every configuration, each its own: (axes [K, 3], offsets [K, M], displacements [K, M, 3], centres [K, M, 2]).  A
    configuration without rows is handed NaN: it reads what a single call without rows reads, whatever they hold."""
    K = sol.n
    _, pos, e1s, e2s, ys = poses(sol, psfd)
    rng = np.random.default_rng(100 * M + seed)
    axes = ys + 0.05 * rng.uniform(-1, 1, (K, 3))
    off = np.linspace(-0.6 * mm, 0.5 * mm, M)[None, :] * (1 + 0.1 * np.arange(K))[:, None] + 0.02 * mm * rng.uniform(-1, 1, (K, 1)) if M > 1 else \
        0.1 * mm * rng.uniform(-1, 1, (K, 1))
    cen = 1e-5 * rng.uniform(-1, 1, (K, M, 2))
    disp = off[:, :, None] * axes[:, None, :] + cen[:, :, 0:1] * e1s[:, None, :] + cen[:, :, 1:2] * e2s[:, None, :]
    for c in range(K):
        if len(rows[c]) == 0:
            axes[c], off[c], cen[c], disp[c] = np.nan, np.nan, np.nan, np.nan
    return axes, np.ascontiguousarray(off), disp, cen


def grid_axes(rows, n):
    """xs, zs [K, n]: a window per configuration, NaN for one without rows"""
    K = len(rows)
    xs = np.linspace(-30e-6, 30e-6, n)[None, :] * (1 + 0.2 * np.arange(K))[:, None] + 1e-6 * np.arange(K)[:, None]
    zs = np.linspace(-24e-6, 33e-6, n)[None, :] * (1 + 0.1 * np.arange(K))[:, None]
    for c in range(K):
        if len(rows[c]) == 0:
            xs[c], zs[c] = np.nan, np.nan
    return xs, zs


def check_shape_of_the_scene(key, rows):
    counts = [len(r) for r in rows]
    print("%r: rows per configuration: %s" % (key, counts))
    if key == "big":
        ns, per = sr.spot_splits(max(counts))
        assert ns == 2 and (max(counts) - per) % 256 != 0 and max(counts) > 2048, (counts, ns, per)  # two row splits, the last tile ragged
    elif key > 1:
        assert 0 in counts and len(set(counts)) >= 3, counts
    return counts


def test_every_configuration_equals_the_single_call(swept):
    key, sol, psfd, rows = swept
    K = sol.n
    counts = check_shape_of_the_scene(key, rows)
    slot, pos, e1s, e2s, _ = poses(sol, psfd)
    for M in PLANES:
        axes, off, disp, _ = planes(sol, psfd, rows, M)
        st, ms = abi.psf_focus_stats_sweep(sol._handle, slot, K, pos, e1s, e2s, axes, off)
        assert st.shape == (K, M, abi.FOCUS_STAT_N) and ms > 0
        for c in range(K):
            want = abi.psf_focus_stats(rows[c], *_pose(sol, psfd, c), axes[c], off[c])[0]
            assert same_bits(st[c], want), (M, c)
            if counts[c] == 0:
                assert (st[c, :, fr.N] == 0).all() and np.isnan(st[c, :, 1:]).all()
            else:
                assert (st[c, :, fr.N] == counts[c]).all() and np.isfinite(st[c]).all()
        for n in GRIDS:
            xs, zs = grid_axes(rows, n)
            I, F, ms = abi.psf_through_focus_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs, want_field=True)
            plain = abi.psf_through_focus_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs)
            assert I.shape == (K, M, n, n) and F.shape == (K, M, n, n) and ms > 0 and plain[1] is None and same_bits(plain[0], I)
            for c in range(K):
                wI, wF, _ = abi.psf_through_focus(rows[c], *_pose(sol, psfd, c), disp[c], xs[c], zs[c], want_field=True)
                assert same_bits(I[c], wI) and same_bits(F[c].real, wF.real) and same_bits(F[c].imag, wF.imag), (M, n, c)
                if counts[c] == 0:
                    assert not I[c].any() and not F[c].any()
                else:
                    assert np.isfinite(I[c]).all() and I[c].max() > 0


def test_rows_parallel_to_the_planes_read_nan_like_the_single_call(swept):
    """Every configuration is read in a frame made for its first row (dx, dy, dz): e1 = (0, 0, 1), e2 = (-dx, -dy, 0) have the normal
    e1 x e2 = (dy, -dx, 0) exactly, so that row's den = (dx * dy + dy * -dx) + dz * 0 is exactly 0: the configuration's statistics and
    transfer function are NaN in the sweep as in the single call."""
    key, sol, psfd, rows = swept
    K = sol.n
    slot, pos, _, _, _ = poses(sol, psfd)
    e1s, e2s, axes = np.tile([0.0, 0.0, 1.0], (K, 1)), np.tile([1.0, 0.0, 0.0], (K, 1)), np.tile([0.0, 1.0, 0.0], (K, 1))
    for c in range(K):
        if len(rows[c]):
            e2s[c] = [-rows[c][0, 3], -rows[c][0, 4], 0.0]
    off = np.tile(np.linspace(-1 * mm, 1 * mm, 9), (K, 1))
    freqs = cp.mtf_frequencies(1e4, 3)
    st = abi.psf_focus_stats_sweep(sol._handle, slot, K, pos, e1s, e2s, axes, off)[0]
    geo = abi.psf_geo_otf_sweep(sol._handle, slot, K, pos, e1s, e2s, axes, off, freqs)
    for c in range(K):
        want = abi.psf_focus_stats(rows[c], pos[c], e1s[c], e2s[c], axes[c], off[c])[0]
        want_geo = abi.psf_geo_otf(rows[c], pos[c], e1s[c], e2s[c], axes[c], off[c], freqs)
        assert same_bits(st[c], want) and same_bits(geo[0][c], want_geo[0]) and same_bits(geo[2][c], want_geo[2]), c
        assert same_bits(geo[1][c].real, want_geo[1].real) and same_bits(geo[1][c].imag, want_geo[1].imag), c
        if len(rows[c]):
            assert (st[c, :, fr.N] == len(rows[c])).all() and np.isnan(st[c, :, 1:]).all()
            assert np.isnan(geo[0][c]).all() and np.isnan(geo[1][c]).all() and np.isnan(geo[2][c]).all()


def test_the_python_methods_equal_the_single_path(swept):
    key, sol, psfd, rows = swept
    K = sol.n
    offsets = np.linspace(-0.4 * mm, 0.4 * mm, 5)
    per_cfg = offsets[None, :] * (1 + 0.1 * np.arange(K))[:, None]
    ori = [np.asarray(sol._poses[c][sol._slot(psfd)][1], dtype=np.float64) for c in range(K)]
    for off_arg, kw in ((offsets, dict()), (per_cfg, dict(follow=None, window_plane=1, crop_factor=3)), (offsets, dict(half_width=2e-5, axis=[0.02, 1.0, -0.01]))):
        xs, zs, d, I, st = sol.psf_through_focus(psfd, off_arg, n=9, **kw)
        assert xs.shape == (K, 9) and d.shape == (K, 5, 3) and I.shape == (K, 5, 9, 9) and st.shape == (K, 5, 12) and sol.readout_ms > 0
        for c in range(K):
            pose = _pose(sol, psfd, c)
            off_c = off_arg if off_arg.ndim == 1 else off_arg[c]
            if len(rows[c]) == 0:
                assert np.isnan(xs[c]).all() and np.isnan(zs[c]).all() and np.isnan(d[c]).all() and not I[c].any()
                assert (st[c, :, fr.N] == 0).all() and np.isnan(st[c, :, 1:]).all()
                continue
            want = cp.psf_through_focus(lambda ax, off: abi.psf_focus_stats(rows[c], *pose, ax, off)[0],
                                        lambda dd, x, z: abi.psf_through_focus(rows[c], *pose, dd, x, z)[0], ori[c], off_c, n=9, **kw)
            for a, b in zip((xs[c], zs[c], d[c], I[c], st[c]), want):
                assert same_bits(a, b), (c, kw)
    st = sol.psf_focus_stats(psfd, per_cfg)
    t, v = sol.psf_best_focus(psfd, per_cfg)
    t_max, v_max = sol.psf_best_focus(psfd, offsets, column=abi.FOCUS_HWX, kind="max")
    assert st.shape == (K, 5, 12) and t.shape == (K,) and v.shape == (K,)
    for c in range(K):
        assert same_bits(st[c], abi.psf_focus_stats(rows[c], *_pose(sol, psfd, c), ori[c][:, 1], per_cfg[c])[0])
        if len(rows[c]) == 0:
            assert np.isnan(t[c]) and np.isnan(v[c]) and np.isnan(t_max[c])
        else:
            assert (t[c], v[c]) == cp.best_focus(per_cfg[c], st[c, :, fr.RMS_R])
            one = abi.psf_focus_stats(rows[c], *_pose(sol, psfd, c), ori[c][:, 1], offsets)[0]
            assert (t_max[c], v_max[c]) == cp.best_focus(offsets, one[:, fr.HWX], kind="max")


def test_detector_only_result_reads_the_same(swept):
    key, sol, psfd, rows = swept
    sol0, psfd0 = make_sweep(key, record_segments=False)
    offsets = np.linspace(-0.4 * mm, 0.4 * mm, 9)
    try:
        for a, b in zip(sol0.psf_through_focus(psfd0, offsets, n=5), sol.psf_through_focus(psfd, offsets, n=5)):
            assert same_bits(a, b)
    finally:
        sol0.close()


def test_a_fresh_solve_of_every_snapshot_reads_the_same():
    """K = 3: block c of SweepSolution.psf_through_focus equals EngineSolution.psf_through_focus after a fresh solve_system of snapshot c."""
    sol, psfd = _sweep(3)
    offsets = np.linspace(-0.4 * mm, 0.4 * mm, 5)
    try:
        got = sol.psf_through_focus(psfd, offsets, n=9, crop_factor=2)
        for c in range(3):
            system, cs, det, lam, D = airy_setup(num_rays=RAYS[3])
            for step in range(c + 1):  # the snapshots of _sweep are cumulative
                x, y = PLACES[3][step]
                bmo.translate_to3d(det, [x, y, 0.0])
                if step > 0:
                    bmo.yrotate3d(det, np.radians(7))
                    bmo.xrotate3d(det, np.radians(0.4))
            bmo.solve_system(system, cs)
            try:
                es = bmo.system._roots_of(cs)[0]._solution
                pos, ori = np.asarray(det.position(), dtype=np.float64), np.asarray(det.orientation(), dtype=np.float64)
                if len(sol.detector_hits(psfd, c)) == 0:
                    with pytest.raises(ValueError, match="recorded no hit"):
                        es.psf_through_focus(0, pos, ori, offsets, n=9, crop_factor=2)
                    continue
                want = es.psf_through_focus(0, pos, ori, offsets, n=9, crop_factor=2)
                for a, b in zip(got, want):
                    assert same_bits(a[c], b), c
            finally:
                bmo.release(cs)
    finally:
        sol.close()


def test_a_stack_of_several_launches():
    """64 configurations of 2 048 rays, n = 100, M = 16: eight splits of 16 x 10 000 partial sums each, 1.3 GB for the sweep, so the
    restated launch rule (readout_ref.sweep_launches) cuts it into at least two launches.  The first and the last configuration and the two
    on either side of the launch boundary equal single calls."""
    K, n, M = 64, 100, 16
    system, cs, psfd, lam, D = airy_setup(num_rays=2048)

    def configure(c):
        bmo.translate_to3d(psfd, [0.0, 200.13 * mm + 0.01 * mm * (c - 32), 0.0])

    sol = bmo.solve_sweep(system, cs, K, configure, record_segments=False)
    try:
        counts = [len(sol.detector_hits(psfd, c)) for c in range(K)]
        splits = [rr.psf_splits(h, n * n)[0] if h else 0 for h in counts]
        launches = rr.sweep_launches(splits, M * n * n)
        assert min(counts) > 0 and len(launches) >= 2 and sum(splits) * M * n * n * 16 > 1 << 30, (counts[:4], launches)
        b = launches[1][0]
        slot, pos, e1s, e2s, ys = poses(sol, psfd)
        off = np.linspace(-0.2 * mm, 0.2 * mm, M)
        disp = off[None, :, None] * ys[:, None, :] + 1e-6 * np.arange(K)[:, None, None] * e1s[:, None, :]
        xs = np.linspace(-40e-6, 40e-6, n)[None, :] + 1e-7 * np.arange(K)[:, None]
        zs = np.tile(np.linspace(-40e-6, 40e-6, n), (K, 1))
        I, _, ms = abi.psf_through_focus_sweep(sol._handle, slot, K, pos, e1s, e2s, disp, xs, zs)
        print("launches %s, kernel %.1f ms" % (launches, ms))
        for c in (0, b - 1, b, K - 1):
            want = abi.psf_through_focus(sol.detector_hits(psfd, c), *_pose(sol, psfd, c), disp[c], xs[c], zs[c])[0]
            assert same_bits(I[c], want) and I[c].max() > 0, c
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------ refusals
def raw(entry, handle, slot, K, null=None, n=4, n_planes=3, n_freqs=2, freqs=None):
    """The return code of one of the four sweep entries on small arguments, `null` naming a pointer argument handed as NULL; a refused
    call must leave every output buffer as it was."""
    lib = abi.load_engine()
    dp = C.POINTER(C.c_double)
    K1, M, nn, nf = max(K, 1), max(n_planes, 1), max(n, 1), max(n_freqs, 1)
    a = dict(origins=np.zeros((K1, 3)), e1s=np.tile([1.0, 0, 0], (K1, 1)), e2s=np.tile([0, 0, 1.0], (K1, 1)), axes=np.tile([0, 1.0, 0], (K1, 1)),
             offsets=np.zeros((K1, M)), displacements=np.zeros((K1, M, 3)), centers=np.zeros((K1, M, 2)), xs=np.tile(np.linspace(-1e-5, 1e-5, nn), (K1, 1)),
             zs=np.tile(np.linspace(-1e-5, 1e-5, nn), (K1, 1)),
             freqs=np.ascontiguousarray(np.tile([1e3, 0.0], (nf, 1)) if freqs is None else np.asarray(freqs, dtype=np.float64)))
    outs = dict(stats=np.full((K1, M, 12), 7.0), out_intensity=np.full((K1, M, nn * nn), 7.0), out_field=np.full((K1, M, nn * nn, 2), 7.0),
                otf=np.full((K1, M, nf, 2), 7.0), mtf=np.full((K1, M, nf), 7.0), sums=np.full((K1, M), 7.0))
    p = {k: (None if k == null else v.ctypes.data_as(dp)) for k, v in {**a, **outs}.items()}
    if entry == "bmo_psf_focus_stats_sweep":
        rc = lib.bmo_psf_focus_stats_sweep(handle, slot, K, p["origins"], p["e1s"], p["e2s"], p["axes"], p["offsets"], n_planes, p["stats"], None)
        used = ("stats",)
    elif entry == "bmo_psf_through_focus_sweep":
        rc = lib.bmo_psf_through_focus_sweep(handle, slot, K, p["origins"], p["e1s"], p["e2s"], p["displacements"], n_planes, p["xs"], p["zs"], n,
                                             p["out_intensity"], p["out_field"], None)
        used = ("out_intensity", "out_field")
    elif entry == "bmo_psf_geo_otf_sweep":
        rc = lib.bmo_psf_geo_otf_sweep(handle, slot, K, p["origins"], p["e1s"], p["e2s"], p["axes"], p["offsets"], p["centers"], n_planes, p["freqs"], n_freqs,
                                       p["otf"], p["mtf"], p["sums"], None)
        used = ("otf", "mtf", "sums")
    else:
        rc = lib.bmo_psf_otf_sweep(handle, slot, K, p["origins"], p["e1s"], p["e2s"], p["displacements"], n_planes, p["xs"], p["zs"], n, p["freqs"], n_freqs,
                                   p["otf"], p["mtf"], p["sums"], p["out_intensity"], None)
        used = ("otf", "mtf", "sums", "out_intensity")
    if rc != 0:
        assert all((v == 7).all() for v in outs.values()), entry
    else:
        assert all(not (outs[k] == 7).any() for k in used if k != null), entry
    return rc


def refusal_sweep():
    """a three-configuration sweep with a PSFDetector and a Spotdetector: (sol, PSF slot, spot slot)"""
    system, cs, psfd, lam, D = airy_setup(num_rays=64)
    spot = bmo.Spotdetector(5 * mm)
    bmo.translate3d(spot, [50 * mm, 0, 0])
    system = bmo.System(list(system.objects()) + [spot])
    p0 = np.array(psfd.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(psfd, list(p0 + np.array([0, 0.1 * mm * c, 0])))

    sol = bmo.solve_sweep(system, cs, 3, configure)
    return sol, psfd, spot


def check_common_refusals(entry, required, sizes):
    """what all four entries refuse: a Spotdetector's slot, a wrong n_configs, a bad slot, a NULL required pointer, sizes <= 0"""
    sol, psfd, spot = refusal_sweep()
    try:
        ps, ss = sol._slot(psfd), sol._slot(spot)
        err = lambda: abi.load_engine().bmo_last_error().decode()  # noqa: E731
        assert raw(entry, sol._handle, ps, 3) == 0
        assert raw(entry, sol._handle, ss, 3) == -1 and "PSFDetector" in err()
        for bad_k in (1, 2, 4, 0):
            assert raw(entry, sol._handle, ps, bad_k) == -1, bad_k
        assert raw(entry, sol._handle, 7, 3) == -1 and raw(entry, sol._handle, -1, 3) == -1
        for name in required:
            assert raw(entry, sol._handle, ps, 3, null=name) == -1 and entry in err(), name
        for name in sizes:
            for bad in (0, -1):
                assert raw(entry, sol._handle, ps, 3, **{name: bad}) == -1 and entry in err(), (name, bad)
        assert raw(entry, None, ps, 3) == -1
    finally:
        sol.close()


def check_a_gaussian_result_is_unsupported(entry):
    import scenes

    system, _ = scenes.c2_scene()
    b = scenes.c3_bundle(64)
    sc = bmo.CompiledScene(system, b.lambdas)
    res, sol = bmo.system._engine_solve(sc, b, 100, None)
    try:
        assert raw(entry, sol.handle, 0, 1) == -4
        assert "GaussianBeamlet" in abi.load_engine().bmo_last_error().decode()
    finally:
        sol.free()


def test_refusals():
    check_common_refusals("bmo_psf_focus_stats_sweep", ("origins", "e1s", "e2s", "axes", "offsets", "stats"), ("n_planes",))
    check_common_refusals("bmo_psf_through_focus_sweep", ("origins", "e1s", "e2s", "displacements", "xs", "zs", "out_intensity"), ("n_planes", "n"))
    sol, psfd, spot = refusal_sweep()
    try:
        assert raw("bmo_psf_through_focus_sweep", sol._handle, sol._slot(psfd), 3, null="out_field") == 0  # optional
        with pytest.raises(RuntimeError, match="bmo_psf_focus_stats_sweep"):
            sol.psf_through_focus(spot, [0.0])
        with pytest.raises(ValueError, match="no offsets"):
            sol.psf_focus_stats(psfd, [])
    finally:
        sol.close()


def test_a_gaussian_result_is_unsupported():
    check_a_gaussian_result_is_unsupported("bmo_psf_focus_stats_sweep")
    check_a_gaussian_result_is_unsupported("bmo_psf_through_focus_sweep")
