"""The oracle's PSF read-out (bmo_cpu_psf_intensity) against a 40-digit evaluation of the reference's formula (PSFDetector.jl:225-232,
tests/readout_ref.py), inside a bound that is derived from the arithmetic and not measured:

    |F_oracle - F_exact| <= (3 u max_h |phase_h| + 2 H u + 8 u) S,    u = 2^-53,  S = sum_h proj_h.

The phase is about 1.3e6 rad, so the bound is about 4.4e-10 S; each case prints its figure ("Read-outs", lists them).
The GPU read-out is then held to the oracle by tests/test_psf_readout.py."""
import numpy as np
import pytest

import bmo_amd as bmo
import readout_ref as rr
from test_psf_readout import airy_setup

mp = pytest.importorskip("mpmath")


def _airy_case(oracle, num_rays, n):
    system, cs, psfd, lam, D = airy_setup(num_rays=num_rays)
    oracle.solve_system(system, cs)
    rows = psfd.data
    assert len(rows) == num_rays
    if num_rays > 1:
        xs, zs = psfd.sample_axes(n=n, crop_factor=5, center="bbox")
    else:
        xs, zs = bmo.linalg.linrange(-1e-5, 1e-5, n), bmo.linalg.linrange(-2e-5, 1e-5, n)
    o = psfd.orientation()
    return rows, np.array(psfd.position(), dtype=np.float64), o[:, 0].copy(), o[:, 2].copy(), xs, zs


def _tilted_case(oracle, num_rays, n):
    system, psfd, bundle = rr.tilted_psf_case(num_rays)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    rows = oracle.trace(scene, bundle, 100).detector_hits(0).copy()
    assert len(rows) == num_rays  # the whole oblique bundle lands on the detector
    pos, o = np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)
    e1, e2 = o[:, 0].copy(), o[:, 2].copy()
    assert np.all(np.abs(e1) > 1e-3) and np.all(np.abs(e2) > 1e-3), (e1, e2)  # no product of p = origin + x e1 + z e2 vanishes
    assert (rows[:, 3:6] != 0).all()  # oblique: every direction component takes part in the dot product
    xs, zs = bmo.components.psf_sample_axes(rows, pos, o, n=n, crop_factor=5, center="bbox")
    return rows, pos, e1, e2, xs, zs


def _check(oracle, case, floor):
    rows, pos, e1, e2, xs, zs = case
    assert len(xs) * len(zs) * len(rows) <= 5e4
    I, F = oracle.psf_intensity(rows, pos, e1, e2, xs, zs)
    exact = rr.psf_field_exact(rows, pos, e1, e2, xs, zs)
    S = float(rows[:, 7].sum())
    phase = rr.psf_max_phase(rows, pos, e1, e2, xs, zs)
    bound = rr.psf_oracle_bound(rows, phase)
    err = float(np.abs(F - exact).max())
    print("H = %d, n = %d: |F_oracle - F_exact| = %.3g S, bound %.3g S, max phase %.3g rad" % (len(rows), len(xs), err / S, bound / S, phase))
    assert phase > 1e5  # the phase term of the bound is the one that counts: ~ 2 pi * 0.2 m / 1 um
    assert err <= bound, (err / S, bound / S)
    # the intensity is the abs2 of that field, rounded: 3 roundings
    assert np.abs(I - (F.real ** 2 + F.imag ** 2)).max() <= 4 * rr.U * float(I.max())
    assert np.abs(I - np.abs(exact) ** 2).max() <= 2 * bound * float(np.abs(exact).max()) + bound * bound + 4 * rr.U * float(I.max())
    if floor:
        assert err > 0.0  # two different computations were compared: a double-precision sum of 10^5 rad phases cannot be exact
    return err / S


@pytest.mark.parametrize("num_rays,n", [(300, 9), (1000, 5)])
def test_oracle_psf_sum_against_exact_on_the_airy_scene(oracle, num_rays, n):
    _check(oracle, _airy_case(oracle, num_rays, n), floor=True)


def test_oracle_psf_sum_against_exact_on_a_tilted_decentred_detector(oracle):
    _check(oracle, _tilted_case(oracle, 400, 9), floor=False)


def test_oracle_psf_sum_against_exact_with_one_hit(oracle):
    rows, pos, e1, e2, xs, zs = case = _airy_case(oracle, 1, 7)
    _check(oracle, case, floor=False)
    # H = 1: |F| = proj at every point, to the rounding of one cis
    _, F = oracle.psf_intensity(rows, pos, e1, e2, xs, zs)
    assert np.abs(np.abs(F) - rows[0, 7]).max() <= 4 * rr.U * rows[0, 7]


def test_psf_splits_restatement_agrees_with_the_header():
    """readout_ref.psf_splits / psf_tiles only tell the GPU tests which path a shape takes; they must use the engine's tile size."""
    assert rr.source_psf_tile() == rr.PSF_TILE == 256
    src = open(rr.READOUT_SOURCE).read()  # the header's comment above psf_splits points here
    assert "n_splits = (4096 + pt_blocks - 1) / pt_blocks;" in src and "n_splits = (2048 + pt_blocks - 1) / pt_blocks;" in src
    for H, pts in [(1, 49), (255, 1), (256, 256), (257, 257), (700, 169), (1000, 250000), (5000, 250000), (1 << 14, 67600), (1 << 18, 49), (1 << 16, 10000)]:
        ns, hps = rr.psf_splits(H, pts)
        tiles = rr.psf_tiles(H, pts)
        assert hps % rr.PSF_TILE == 0 and hps >= rr.PSF_TILE
        assert 1 <= ns <= 65535 and (ns - 1) * hps < H <= ns * hps  # no empty split, every hit in one
        assert len(tiles) == ns and sum(map(sum, tiles)) == H
    assert rr.psf_splits(0, 49) == (1, 256) and rr.psf_tiles(0, 49) == [[]]
    # the shapes tests/test_psf_readout.py had before: never a second tile in a split
    for H, n in [(1000, 500), (300, 33), (1, 7)]:
        assert max(len(t) for t in rr.psf_tiles(H, n * n)) == 1
    assert rr.psf_tiles(5000, 250000) == [[256] * 4] * 4 + [[256, 256, 256, 136]]
    assert rr.psf_splits(1 << 18, 49) == (1024, 256)
    # pd_splits: ranges of beamlets, no tile
    assert rr.pd_splits(1, 2304) == (1, 1) and rr.pd_splits(228, 2304) == (228, 1) and rr.pd_splits(300, 2304) == (150, 2)
    assert rr.pd_splits(358, 4096) == (120, 3) and rr.pd_splits(3, 1) == (3, 1)


def test_sweep_launches_restatement_on_the_shapes_the_gpu_tests_use():
    """readout_ref.sweep_launches restates SplitPlan's launch rule; the two sweeps the GPU tests split into three launches, by hand."""
    src = open(rr.READOUT_SOURCE).read()
    assert src.count("((int64_t)1 << 30) / (n_pts * 16)") == 1 and "std::min<int64_t>(65535, ((int64_t)1 << 30)" in src  # the one limit
    # Photodetector (test_more_configurations_than_one_launch_holds): 260 configurations x 228 beamlets on 48 x 48 points.  9 point blocks ask
    # for cdiv(2048, 9) = 228 ranges: one beamlet each.  2^30 // (2304 * 16) = 29127 rows, 29127 // 228 = 127 configurations per launch.
    assert rr.pd_splits(228, 48 * 48) == (228, 1) and (1 << 30) // (48 * 48 * 16) == 29127 and 29127 // 228 == 127
    assert rr.sweep_launches([228] * 260, 48 * 48) == [(0, 127), (127, 127), (254, 6)]
    # PSF (test_psf_sweep_gpu's three-launch sweep): 150 configurations of 16 splits on 256 x 256 points.  2^30 / 2^20 = 1024 rows, 64 per launch.
    assert (1 << 30) // (256 * 256 * 16) == 1024
    assert rr.sweep_launches([16] * 150, 256 * 256) == [(0, 64), (64, 64), (128, 22)]
    # unequal counts pack by rows, not by the largest configuration; empty configurations take no row; an oversized one goes alone
    assert rr.sweep_launches([600, 0, 400, 24, 1, 1000, 24], 256 * 256) == [(0, 4), (4, 2), (6, 1)]
    assert rr.sweep_launches([5, 2000, 5], 256 * 256) == [(0, 1), (1, 1), (2, 1)]
    assert rr.sweep_launches([0, 0, 0], 49) == [(0, 3)] and rr.sweep_launches([], 49) == []
    assert rr.sweep_launches([0] * 70000, 49) == [(0, 65535), (65535, 4465)]  # at most 65535 configurations (grid y of the reduction)
    assert rr.sweep_launches([1] * 70000, 16) == [(0, 65535), (65535, 4465)]  # ... and 65535 rows (grid y of the accumulation)
