"""Spotdetector read-out of sweeps on the GPU: SweepSolution.spot_image / spot_stats (bmo_spot_image_sweep / bmo_spot_stats_sweep) equal,
configuration by configuration, the single calls on that configuration's rows: images exactly, statistics bit for bit."""

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
import spot_ref as sr

pytestmark = pytest.mark.gpu
mm = 1e-3


def _same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def test_unequal_and_empty_configurations():
    """A 4 mm detector in a 15 mm collimated beam, moved sideways: the row counts differ and configuration 3 records no hit."""
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 15 * mm, 1e-6, num_rays=2000, e1=[1, 0, 0])
    sd = bmo.Spotdetector(4 * mm)
    bmo.translate3d(sd, [0, 50 * mm, 0])
    system = bmo.System([sd])
    xoff = [0.0, 3 * mm, 5.5 * mm, 30 * mm]

    def configure(c):
        bmo.translate_to3d(sd, [xoff[c], 50 * mm, 0])

    sol = bmo.solve_sweep(system, cs, len(xoff), configure)
    try:
        K = len(xoff)
        rows = [sol.spot_hits(sd, c) for c in range(K)]
        counts = [len(r) for r in rows]
        assert counts[3] == 0 and len(set(counts[:3])) == 3 and min(counts[:3]) > 0, counts
        nx, nz = 24, 10
        per_cfg = np.array([[-2 * mm, 2 * mm, -2 * mm, 2 * mm], [-2 * mm, 0.5 * mm, -1 * mm, 2 * mm], [-1 * mm, 1 * mm, -0.3 * mm, 0.2 * mm],
                            [-2 * mm, 2 * mm, -2 * mm, 2 * mm]])
        shared = (-1.5 * mm, 2 * mm, -2 * mm, 1 * mm)
        for windows in (per_cfg, shared):
            w, img, outside = sol.spot_image(sd, nx, nz, window=windows)
            assert w.shape == (K, 4) and img.shape == (K, nx, nz) and outside.shape == (K,) and sol.readout_ms > 0
            for c in range(K):
                one, one_out, _ = abi.spot_image(rows[c], w[c], nx, nz)
                want, want_out = sr.bin_rule(rows[c], w[c], nx, nz)
                assert np.array_equal(img[c], one) and np.array_equal(img[c], want), c
                assert outside[c] == one_out == want_out and img[c].sum() + outside[c] == counts[c], c
            assert not img[3].any() and outside[3] == 0
        # window = None is the detector face
        w, img, outside = sol.spot_image(sd, 8)
        assert np.array_equal(w, np.tile([-2 * mm, 2 * mm, -2 * mm, 2 * mm], (K, 1))) and img.shape == (K, 8, 8)
        assert [int(img[c].sum() + outside[c]) for c in range(K)] == counts
        st = sol.spot_stats(sd)
        assert st.shape == (K, 12)
        for c in range(K):
            one, _ = abi.spot_stats(rows[c])
            assert _same_bits(st[c], one), c
            assert sr.stat_violations(st[c], rows[c]) == [], c
        assert st[3, sr.N] == 0 and np.isnan(st[3, 1:]).all()
        with pytest.raises(ValueError, match="configuration 3"):
            sol.spot_image(sd, nx, nz, window="extent")
    finally:
        sol.close()


def _through_focus(K, num_rays):
    lens = bmo.SphericalLens(100 * mm, float("inf"), 1 * mm, 25.4 * mm, lambda lam_: 1.5)
    sd = bmo.Spotdetector(4 * mm)
    system = bmo.System([lens, sd])
    cs = bmo.UniformDiscSource([0, -10 * mm, 0], [0, 1, 0], 10 * mm, 1e-6, num_rays=num_rays)
    ys = bmo.linalg.linrange(185 * mm, 215 * mm, K)  # the paraxial focus of the plano-convex lens is 200 mm behind it

    def configure(c):
        bmo.translate_to3d(sd, [0, ys[c], 0])

    return system, cs, sd, lens, ys, configure


def test_through_focus_scan():
    K = 9
    system, cs, sd, lens, ys, configure = _through_focus(K, 1000)
    sol = bmo.solve_sweep(system, cs, K, configure)
    try:
        st = sol.spot_stats(sd)
        for c in range(K):
            rows = sol.spot_hits(sd, c)
            assert len(rows) == 1000
            assert sr.stat_violations(st[c], rows) == [], c
        assert int(st[:, sr.RMS_R].argmin()) not in (0, K - 1), st[:, sr.RMS_R]
        w, img, outside = sol.spot_image(sd, 32, window="extent")
        for c in range(K):
            assert tuple(w[c]) == tuple(st[c, sr.X_MIN:sr.Z_MAX + 1]) and outside[c] == 0 and img[c].sum() == 1000
            assert np.array_equal(img[c], sr.bin_rule(sol.spot_hits(sd, c), w[c], 32, 32)[0])
        # a fresh solve of snapshot c, read the way a user reads one spot diagram
        for c in range(K):
            system2, cs2, sd2, _, _, configure2 = _through_focus(K, 1000)
            configure2(c)
            bmo.solve_system(system2, cs2)
            assert _same_bits(sd2.stats(), st[c]), c
            bmo.release(cs2)
    finally:
        sol.close()


def test_detector_only_sweep_reads_the_same():
    K = 5
    system, cs, sd, lens, ys, configure = _through_focus(K, 700)
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scenes_, poses, grids = bmo.system.sweep_snapshots(system, bundle.lambdas, K, configure)
    tiled = bmo.RayBundle(bundle.kind, np.tile(bundle.planes, (1, K)))
    cfg = np.repeat(np.arange(K, dtype=np.int32), bundle.n)
    slot = [i for i, d in enumerate(scenes_[0].detectors) if d is sd][0]
    window = (-1 * mm, 1 * mm, -1 * mm, 1 * mm)
    got = []
    for record in (True, False):
        _, h, lib = bmo.system.sweep_trace(scenes_, tiled, cfg, record_segments=record, view=False)
        try:
            img, outside, _ = abi.spot_image_sweep(h, slot, K, window, 40, 24)
            st, _ = abi.spot_stats_sweep(h, slot, K)
            got.append((img, outside, st))
        finally:
            lib.bmo_result_free(h)
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]) and _same_bits(got[0][2], got[1][2])
    assert (got[0][2][:, sr.N] == 700).all() and got[0][0].sum() + got[0][1].sum() == K * 700


def test_splits_across_configurations():
    """Three runs of roots of unequal length: the middle configuration has at least three splits with a ragged last, its neighbours one."""
    n_mid = sr.smallest_ragged_three_splits()
    runs = [300, n_mid, 1000]
    assert [sr.spot_splits(n)[0] for n in runs] == [1, sr.spot_splits(n_mid)[0], 1] and sr.spot_splits(n_mid)[0] >= 3 and n_mid % sr.spot_splits(n_mid)[1]
    K = len(runs)
    system, cs, sd, lens, ys, configure = _through_focus(K, sum(runs))
    bundle = bmo.RayBundle.from_beams(cs.beams)
    scenes_, poses, grids = bmo.system.sweep_snapshots(system, bundle.lambdas, K, configure)
    cfg = np.repeat(np.arange(K, dtype=np.int32), runs)
    res, h, lib = bmo.system.sweep_trace(scenes_, bundle, cfg)
    try:
        slot = 0
        rows_all = res.detector_hits(slot)[:, 0:2]
        row_cfg = cfg[res.node_root[res.detector_nodes(slot)]]
        assert [int((row_cfg == c).sum()) for c in range(K)] == runs  # every ray reaches the detector
        windows = np.array([[-1 * mm, 1 * mm, -1 * mm, 1 * mm], [-0.5 * mm, 0.5 * mm, -0.2 * mm, 0.6 * mm], [-2 * mm, 2 * mm, -2 * mm, 2 * mm]])
        for nx, nz in ((33, 17), (129, 128)):
            img, outside, _ = abi.spot_image_sweep(h, slot, K, windows, nx, nz)
            for c in range(K):
                rows = rows_all[row_cfg == c]
                one, one_out, _ = abi.spot_image(rows, windows[c], nx, nz)
                assert np.array_equal(img[c], one) and outside[c] == one_out, (c, nx, nz)
                assert np.array_equal(img[c], sr.bin_rule(rows, windows[c], nx, nz)[0]), (c, nx, nz)
        st, _ = abi.spot_stats_sweep(h, slot, K)
        for c in range(K):
            rows = rows_all[row_cfg == c]
            assert _same_bits(st[c], abi.spot_stats(rows)[0]), c
            assert sr.stat_violations(st[c], rows) == [], c
    finally:
        lib.bmo_result_free(h)
