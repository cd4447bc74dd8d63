"""Photodetector read-out of sweeps on the GPU: configuration c of bmo_photodetector_field_sweep equals, bit for bit, a fresh solve of snapshot c
followed by bmo_photodetector_field at that snapshot's detector pose; a few configurations per test are also held to the oracle.  The cases
are the ones tests/test_sweep_gpu.py's Michelson KAT leaves out: a detector pose per configuration, unequal and empty configurations, several
beamlets per range, more configurations than one launch holds, ragged counts across a launch boundary, accumulation into the caller's field,
a non-square grid, and the refusals.  The sweep and the single call share their device code: the independent check is the oracle's."""
import ctypes as C
import math

import numpy as np
import pytest

import bmo_amd as bmo
import readout_ref as rr
import scenes
from bmo_amd import abi
from bmo_amd.system import _engine_solve
from test_photodetector import pd_scene

pytestmark = pytest.mark.gpu
mm = 1e-3
R_MAX = 20
DP = C.POINTER(C.c_double)


class _Sweep:
    """K snapshots of `system` (configure(c) before each), `bundle` traced in every one of them by one bmo_trace_sweep."""

    def __init__(self, system, pd, bundle, K, configure, record_segments=True):
        self.bundle, self.K, self.pd = bundle, K, pd
        self.scenes, self.poses, _ = bmo.sweep_snapshots(system, bundle.lambdas, K, configure)
        self.slot = next(i for i, d in enumerate(self.scenes[0].detectors) if d is pd)
        tiled = bmo.RayBundle(bundle.kind, np.tile(bundle.planes, (1, K)))
        self.res, self.handle, self.lib = bmo.sweep_trace(self.scenes, tiled, np.repeat(np.arange(K, dtype=np.int32), bundle.n), R_MAX, 0, record_segments)
        cfg = self.res.node_root[self.res.detector_nodes(self.slot)] // bundle.n
        self.counts = [int(v) // 3 for v in np.bincount(cfg, minlength=K)]  # recorded beamlets per configuration (three rows each)
        self.pos = np.ascontiguousarray([self.poses[c][self.slot][0] for c in range(K)], dtype=np.float64)
        self.ori = np.ascontiguousarray([np.asarray(self.poses[c][self.slot][1]).reshape(9) for c in range(K)], dtype=np.float64)

    def close(self):
        if self.handle:
            self.lib.bmo_result_free(self.handle)
            self.handle = None

    def raw(self, buf, xs, ys, slot=None, K=None, nx=None, ny=None, null=()):
        """bmo_photodetector_field_sweep's return code; buf: float64 [K * nx * ny * 2], (c, i, j) at 2 * (c * nx * ny + i + nx * j)."""
        x, y = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
        args = dict(pos=self.pos.ctypes.data_as(DP), ori=self.ori.ctypes.data_as(DP), xs=x.ctypes.data_as(DP), ys=y.ctypes.data_as(DP),
                    field=buf.ctypes.data_as(DP))
        for name in null:
            args[name] = None
        return self.lib.bmo_photodetector_field_sweep(None if "res" in null else self.handle, self.slot if slot is None else slot, self.K if K is None else K,
                                                      args["pos"], args["ori"], args["xs"], args["ys"], len(x) if nx is None else nx,
                                                      len(y) if ny is None else ny, args["field"], None)

    def fields(self, xs, ys, start=None):
        """[K, nx, ny] complex: the sweep read-out added to `start` (zeros without it)."""
        nx, ny = len(xs), len(ys)
        buf = np.zeros(2 * self.K * nx * ny)
        if start is not None:
            st = np.ascontiguousarray(start.transpose(0, 2, 1)).reshape(-1)
            buf[0::2], buf[1::2] = st.real, st.imag
        rc = self.raw(buf, xs, ys)
        assert rc == 0, (rc, self.lib.bmo_last_error())
        return np.ascontiguousarray((buf[0::2] + 1j * buf[1::2]).reshape(self.K, ny, nx).transpose(0, 2, 1))

    def single(self, c, xs, ys):
        """A fresh solve of snapshot c + bmo_photodetector_field at its pose."""
        res, one = _engine_solve(self.scenes[c], self.bundle, R_MAX, None)
        try:
            assert res.det_count[self.slot] == 3 * self.counts[c], c
            f = np.zeros((len(xs), len(ys)), dtype=np.complex128)
            one.photodetector_field(self.slot, self.poses[c][self.slot][0], self.poses[c][self.slot][1], xs, ys, f)
        finally:
            one.free()
        return f

    def oracle_field(self, oracle, c, xs, ys):
        a, osol = oracle.trace(self.scenes[c], self.bundle, R_MAX, threads=16, keep=True)
        try:
            assert a.det_count[self.slot] == 3 * self.counts[c], c
            f = np.zeros((len(xs), len(ys)), dtype=np.complex128)
            osol.photodetector_field(self.slot, self.poses[c][self.slot][0], self.poses[c][self.slot][1], xs, ys, f)
        finally:
            osol.free()
        return f


def _same_bits(a, b):
    return a.shape == b.shape and bool((np.ascontiguousarray(a).view(np.int64) == np.ascontiguousarray(b).view(np.int64)).all())


def _moving_sweep(n, K, step=1.0):
    """pd_scene's train; the Photodetector is translated and tilted differently in every configuration."""
    system, pd, bundle = pd_scene(n)
    p0 = np.array(pd.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(pd, list(p0 + step * np.array([0.02 * mm * c, -0.015 * mm * ((c * 3) % 5), 0.1 * mm * (c % 4)])))
        bmo.xrotate3d(pd, math.radians(0.7 * step * (1 + c % 3)))
        bmo.zrotate3d(pd, math.radians(-0.5 * step * (1 + c % 2)))

    return _Sweep(system, pd, bundle, K, configure), pd


def test_moving_detector_every_configuration_reads_at_its_own_pose(oracle):
    K = 6
    sw, pd = _moving_sweep(40, K)
    try:
        assert sw.counts == [40] * K
        f = sw.fields(pd.x, pd.y)
        assert f.shape == (K, len(pd.x), len(pd.y))
        peak = np.abs(f).max()
        for c in range(K):
            for d in range(c):  # a pose mix-up cannot pass: any two configurations differ visibly, in pose and in field
                assert np.abs(sw.pos[c] - sw.pos[d]).max() > 1e-6 and np.abs(sw.ori[c] - sw.ori[d]).max() > 1e-3
                assert np.abs(f[c] - f[d]).max() > 1e-3 * peak, (c, d)
            assert _same_bits(f[c], sw.single(c, pd.x, pd.y)), c
        for c in (0, 3, K - 1):
            fa = sw.oracle_field(oracle, c, pd.x, pd.y)
            assert np.abs(f[c] - fa).max() <= 1e-9 * np.abs(fa).max(), c
    finally:
        sw.close()


def _ragged_sweep():
    """A 4.5 mm Photodetector (64 x 64 points) moved sideways through a 12 mm bundle of 2 000 collimated beamlets: configuration 2 records
    none, the others between a few and a few hundred."""
    bundle = scenes.gaussian_bundle(2000, center=[0, 0, 0], direction=[0, 1, 0], diameter=12 * mm, lam=1e-6, w0=0.2 * mm, jitter=1e-3)
    pd = bmo.Photodetector(4.5 * mm, 64)
    bmo.translate3d(pd, [0, 50 * mm, 0])
    xoff = [0.0, 5.0 * mm, 40 * mm, 7.6 * mm, 6.5 * mm]

    def configure(c):
        bmo.translate_to3d(pd, [xoff[c], 50 * mm, 0.2 * mm * c])

    return _Sweep(bmo.System([pd]), pd, bundle, len(xoff), configure), pd


def test_unequal_and_empty_configurations(oracle):
    sw, pd = _ragged_sweep()
    try:
        n_pts = len(pd.x) * len(pd.y)
        K, counts = sw.K, sw.counts
        assert counts[2] == 0 and min(counts[c] for c in (0, 1, 3, 4)) > 0 and len(set(counts)) == K, counts
        splits = [rr.pd_splits(h, n_pts) if h else (0, 0) for h in counts]
        assert len({s[0] for s in splits}) >= 4, splits            # the split counts differ: rows past a configuration's own count return early
        assert len({s[1] for s in splits if s[0]}) >= 3, splits    # ... and so do the beamlets per range,
        assert max(s[1] for s in splits) > 1 and min(s[1] for s in splits if s[0]) == 1, splits  # some above one, some one
        f = sw.fields(pd.x, pd.y)
        assert not f[2].real.any() and not f[2].imag.any()  # nothing recorded, zeros passed: exactly zero
        for c in range(K):
            assert _same_bits(f[c], sw.single(c, pd.x, pd.y)), c
        for c in (0, 3):
            fa = sw.oracle_field(oracle, c, pd.x, pd.y)
            assert np.abs(fa).max() > 0 and np.abs(f[c] - fa).max() <= 1e-9 * np.abs(fa).max(), c
    finally:
        sw.close()


def test_accumulation_into_the_callers_field():
    sw, pd = _ragged_sweep()
    try:
        f = sw.fields(pd.x, pd.y)
        rng = np.random.Generator(np.random.PCG64(7))
        # a second call on the returned buffer doubles every configuration
        f2 = sw.fields(pd.x, pd.y, start=f)
        for c in range(sw.K):
            peak = np.abs(f[c]).max()
            assert np.abs(f2[c] - 2 * f[c]).max() <= 1e-12 * peak, c
            assert (peak > 0) == (sw.counts[c] > 0)
        # a non-zero start: added to where beamlets were recorded, returned unchanged where none was
        start = (rng.standard_normal(f.shape) + 1j * rng.standard_normal(f.shape)) * np.abs(f).max()
        f3 = sw.fields(pd.x, pd.y, start=start)
        assert sw.counts[2] == 0 and _same_bits(f3[2], start[2])
        for c in (0, 1, 3, 4):
            assert np.abs(f3[c] - (start[c] + f[c])).max() <= 1e-12 * np.abs(start).max(), c
            assert np.abs(f3[c] - start[c]).max() > 0
    finally:
        sw.close()


def test_more_configurations_than_one_launch_holds(oracle):
    """260 configurations x 228 beamlets on pd_scene's 48 x 48 grid: 228 ranges and 8.4 MB of partial sums per configuration, so the 1 GiB cap
    of one launch makes it three (first configurations 0, 127, 254)."""
    K, n = 260, 228
    sw, pd = _moving_sweep(n, K, step=0.01)
    try:
        n_pts = len(pd.x) * len(pd.y)
        assert sw.counts == [n] * K and sum(sw.counts) <= 1e5
        launches = rr.sweep_launches([rr.pd_splits(h, n_pts)[0] for h in sw.counts], n_pts)
        assert len(launches) == 3 and [c0 for c0, _ in launches] == [0, 127, 254], launches
        batch = launches[1][0]
        f = sw.fields(pd.x, pd.y)
        check = {0, 1, K - 2, K - 1}
        for b, _ in launches[1:]:
            check |= {b - 1, b, b + 1}
        assert len(check) >= 10
        for c in sorted(check):
            assert _same_bits(f[c], sw.single(c, pd.x, pd.y)), c
        for c in (batch, K - 1):
            fa = sw.oracle_field(oracle, c, pd.x, pd.y)
            assert np.abs(f[c] - fa).max() <= 1e-9 * np.abs(fa).max(), c
        # neighbours across a launch boundary are different configurations
        assert not _same_bits(f[batch - 1], f[batch]) and not _same_bits(f[2 * batch - 1], f[2 * batch])
    finally:
        sw.close()


def test_ragged_counts_across_a_launch_boundary(oracle):
    """_ragged_sweep's detector with 48 x 48 points, stepped through a bundle of 1 200 beamlets 280 times: inside the bundle it records about
    two hundred beamlets, towards the rim fewer, every tenth configuration none.  A launch holds 2^30 // (2304 * 16) = 29 127 ranges whichever
    configurations they belong to: two launches, where one sized by the largest configuration (the rule before) took three."""
    K = 280
    bundle = scenes.gaussian_bundle(1200, center=[0, 0, 0], direction=[0, 1, 0], diameter=12 * mm, lam=1e-6, w0=0.2 * mm, jitter=1e-3)
    pd = bmo.Photodetector(4.5 * mm, 48)
    bmo.translate3d(pd, [0, 50 * mm, 0])
    xoff = [0.0, 5.0 * mm, 2.0 * mm, 40 * mm, 1.0 * mm, 6.5 * mm, 3.0 * mm, -1.5 * mm, 7.6 * mm, -2.5 * mm]

    def configure(c):
        bmo.translate_to3d(pd, [xoff[c % 10] + 0.0005 * mm * c, 50 * mm, 0.005 * mm * c])

    sw = _Sweep(bmo.System([pd]), pd, bundle, K, configure)
    try:
        n_pts = len(pd.x) * len(pd.y)
        counts = sw.counts
        assert n_pts == 48 * 48 and sum(counts) <= 1e5
        empty = [c for c in range(K) if counts[c] == 0]
        assert empty == list(range(3, K, 10)) and len(set(counts)) >= 20, counts
        splits = [rr.pd_splits(h, n_pts)[0] if h else 0 for h in counts]
        launches = rr.sweep_launches(splits, n_pts)
        old_batch = max(1, min(K, 65535, (1 << 30) // (max(splits) * n_pts * 16)))  # the rule before: every configuration as many rows as the largest
        old_starts = list(range(old_batch, K, old_batch))
        assert len(launches) == 2 and len(old_starts) + 1 == 3, (launches, old_batch)
        new_starts = [c0 for c0, _ in launches[1:]]
        assert not set(new_starts) & set(old_starts)
        f = sw.fields(pd.x, pd.y)
        check = {0, K - 1}
        for b in new_starts + old_starts:
            check |= {b - 1, b}
        near = min(empty, key=lambda c: abs(c - new_starts[0]))  # the empty configuration next to the new boundary
        check |= {near - 1, near, near + 1}
        assert len(check) >= 10
        for c in sorted(check):
            assert _same_bits(f[c], sw.single(c, pd.x, pd.y)), c
        assert not f[near].real.any() and not f[near].imag.any()
        assert not _same_bits(f[new_starts[0] - 1], f[new_starts[0]])
        c = new_starts[0] if counts[new_starts[0]] else new_starts[0] - 1
        fa = sw.oracle_field(oracle, c, pd.x, pd.y)
        assert np.abs(fa).max() > 0 and np.abs(f[c] - fa).max() <= 1e-9 * np.abs(fa).max(), c
    finally:
        sw.close()


def test_non_square_grid(oracle):
    K = 4
    sw, pd = _moving_sweep(40, K)
    try:
        xs = bmo.linalg.linrange(-0.30 * mm, 0.45 * mm, 40)
        ys = bmo.linalg.linrange(-0.25 * mm, 0.40 * mm, 9)
        f = sw.fields(xs, ys)
        assert f.shape == (K, 40, 9) and np.abs(f).max() > 0
        for c in range(K):
            assert _same_bits(f[c], sw.single(c, xs, ys)), c
        fa = sw.oracle_field(oracle, 2, xs, ys)
        assert np.abs(f[2] - fa).max() <= 1e-9 * np.abs(fa).max()
    finally:
        sw.close()


def test_refusals():
    K = 3
    sw, pd = _moving_sweep(5, K)
    try:
        nx, ny = len(pd.x), len(pd.y)
        mark = np.arange(2 * K * nx * ny, dtype=np.float64) + 0.5
        buf = mark.copy()

        def refused(**kw):
            rc = sw.raw(buf, pd.x, pd.y, **kw)
            assert np.array_equal(buf, mark), kw  # a refused call leaves the caller's field alone
            return rc == -1 and b"bmo_photodetector_field_sweep" in sw.lib.bmo_last_error()

        for bad_k in (0, K - 1, K + 1):
            assert refused(K=bad_k), bad_k
        for bad_slot in (-1, len(sw.scenes[0].detectors), 99):
            assert refused(slot=bad_slot), bad_slot
        for name in ("res", "pos", "ori", "xs", "ys", "field"):
            assert refused(null=(name,)), name
        assert refused(nx=0) and refused(ny=0) and refused(nx=-1)
        assert sw.raw(buf, pd.x, pd.y) == 0 and not np.array_equal(buf, mark)  # and the same call with good arguments is served
    finally:
        sw.close()


def test_result_without_segments_is_refused():
    system, pd, bundle = pd_scene(5)
    sw = _Sweep(system, pd, bundle, 2, lambda c: bmo.translate3d(pd, [0.01 * mm, 0, 0]), record_segments=False)
    try:
        assert sw.counts == [5, 5]  # the hits are recorded, the segments gauss_parameters needs are not
        mark = np.arange(2 * 2 * 48 * 48, dtype=np.float64)
        buf = mark.copy()
        assert sw.raw(buf, pd.x, pd.y) == -1
        assert b"record_segments" in sw.lib.bmo_last_error()
        assert np.array_equal(buf, mark)
    finally:
        sw.close()


def test_ray_sweep_leaves_the_field_untouched():
    """Plain rays leave no record on a Photodetector (Photodetector.jl:57-60): the call succeeds and adds nothing."""
    system, pd, _ = pd_scene(1)
    bundle = scenes.c2_bundle(50)
    sw = _Sweep(system, pd, bundle, 3, lambda c: bmo.translate3d(pd, [0.01 * mm, 0, 0]))
    try:
        mark = np.arange(2 * 3 * 48 * 48, dtype=np.float64) - 7.25
        buf = mark.copy()
        assert sw.raw(buf, pd.x, pd.y) == 0
        assert np.array_equal(buf, mark)
        assert sw.raw(buf, pd.x, pd.y, K=4) == -1  # the configuration count is checked all the same
    finally:
        sw.close()
