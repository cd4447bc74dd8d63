"""The GPU's Photodetector read-out on the scenes of tests/test_pd_field_reference.py, which enter what no other Photodetector scene enters:
pd_locate's earlier-segment walk, a child beamlet read at z < length(parent), a grid across a focus, and a sum over three wavelengths
(pd_tables -> pd_prepare_kernel -> pd_locate -> gauss_parameters_at -> pd_field_range in csrc/bmo_readout.inc.hpp).  The engine is held

  - to the oracle within TAIL_ULPS ulp of sum_h |E_h| at every point (the derivation beside TAIL_ULPS in tests/test_photodetector.py covers these
    scenes unchanged: z, r, w, R, psi, ph and ref_phi are the same doubles on both sides, only exp and sincos differ), and
  - to the 50-digit evaluation of the reference's formulas within pd_ref's derived bound plus those TAIL_ULPS ulp (where mpmath imports).

The sweep read-out equals the single one bit for bit, and bmo_gauss_parameters at the z values of these grids equals the oracle's
gauss_parameters exactly: the premise of the ulp bound, asserted."""
import numpy as np
import pytest

import bmo_amd as bmo
import pd_ref
from parity import compare
from test_photodetector import TAIL_FLOOR, TAIL_ULPS
from test_photodetector_sweep_gpu import _same_bits, _Sweep

pytestmark = pytest.mark.gpu
R_MAX = 20
NAMES = list(pd_ref.SCENES)


class _Engine:
    def __init__(self, c):
        self.res, self.sol = bmo.system._engine_solve(c.scene, c.bundle, R_MAX, None)
        self.field = np.zeros_like(c.oracle_field)
        self.sol.photodetector_field(c.slot, c.position, c.orientation, c.xs, c.ys, self.field)


@pytest.fixture(scope="module")
def solved(oracle):
    """name -> (the oracle's case, the engine's solve and field of it), solved once per module."""
    cache = {}

    def get(name):
        if name not in cache:
            c = pd_ref.solved_case(oracle, name)
            cache[name] = (c, _Engine(c))
        return cache[name]

    yield get
    for _, e in cache.values():
        e.sol.free()


def _scale(oracle, c):
    """sum_h |E_h| [nx, ny] out of the oracle, one root beamlet at a time (every scene here records at most one beamlet per root)."""
    if len(c.records) == 1:
        return np.abs(c.oracle_field)
    scale, total = np.zeros(c.oracle_field.shape), np.zeros_like(c.oracle_field)
    for h in range(c.bundle.n):
        one = bmo.RayBundle(c.bundle.kind, c.bundle.planes[:, h:h + 1].copy())
        a1, osol1 = oracle.trace(c.scene, one, R_MAX, keep=True)
        assert a1.det_count[c.slot] == 3
        f1 = np.zeros_like(c.oracle_field)
        osol1.photodetector_field(c.slot, c.position, c.orientation, c.xs, c.ys, f1)
        osol1.free()
        scale += np.abs(f1)
        total += f1
    assert (np.abs(total - c.oracle_field) <= 4 * 2.0 ** -52 * scale).all()  # the read-outs are the terms of the sum
    return scale


@pytest.mark.parametrize("name", NAMES)
def test_trace_and_field_against_the_oracle(oracle, solved, name):
    c, e = solved(name)
    compare(e.res, c.res, 0.0, name)
    assert c.res.det_count[c.slot] == 3 * len(c.records) and c.oracle_field.size <= 441 and len(c.records) <= 3
    fa, fg = c.oracle_field, e.field
    assert np.isfinite(fa.view(np.float64)).all() and np.isfinite(fg.view(np.float64)).all() and np.abs(fa).max() > 0
    scale = _scale(oracle, c)
    live = scale > TAIL_FLOOR
    assert live.mean() >= 0.9, live.mean()
    rel = np.abs(fg - fa)[live] / scale[live]
    print("%s: %d points, %.0f %% live, min scale / peak %.3g, engine - oracle at most %.2f ulp of sum|E_h|" % (name, fa.size, 100 * live.mean(), scale.min() / scale.max(), rel.max() * 2.0 ** 52))
    assert rel.max() <= TAIL_ULPS * 2.0 ** -52, rel.max() * 2.0 ** 52


@pytest.mark.parametrize("name", NAMES)
def test_field_against_the_exact_evaluation(oracle, solved, name):
    pytest.importorskip("mpmath")
    c, e = solved(name)
    ex = pd_ref.pd_case(oracle, name).exact
    live = ex.scale > TAIL_FLOOR
    assert live.mean() >= 0.9, live.mean()
    err = ex.error(e.field)
    tol = ex.bound + TAIL_ULPS * 2.0 ** -52 * ex.scale
    print("%s: engine - exact at most %.3g of the tolerance, %.3g of sum|E_h|" % (name, (err[live] / tol[live]).max(), (err[live] / ex.scale[live]).max()))
    assert (err[live] <= tol[live]).all(), (err[live] / tol[live]).max()
    assert err.max() > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_the_call_adds_to_the_callers_field(oracle, solved, name):
    c, e = solved(name)
    start = (np.arange(e.field.size, dtype=np.float64).reshape(e.field.shape) % 7 - 3) * (1 + 0.5j) * np.abs(e.field).max()
    got = start.copy()
    e.sol.photodetector_field(c.slot, c.position, c.orientation, c.xs, c.ys, got)
    assert _same_bits(got, start + e.field)  # the reduction adds the finished sum to the caller's value: one rounding, the same here
    twice = e.field.copy()
    e.sol.photodetector_field(c.slot, c.position, c.orientation, c.xs, c.ys, twice)
    assert _same_bits(twice, 2 * e.field)


def test_sweep_equals_single_on_the_steep_and_the_untilted_pose(oracle):
    """Two configurations of the earlier-segment scene: its steep pose, where pd_locate walks the segments, and the same detector untilted, where
    every point stays on the last segment."""
    system, pd, roots, xs, ys = pd_ref.SCENES["earlier_segment"]()
    bundle = bmo.RayBundle.from_beams(roots)
    sw = _Sweep(system, pd, bundle, 2, lambda k: bmo.reset_rotation3d(pd) if k == 1 else None)
    try:
        assert sw.counts == [1, 1]
        assert np.abs(sw.ori[0] - sw.ori[1]).max() > 0.5 and np.array_equal(sw.pos[0], sw.pos[1])
        assert np.array_equal(sw.ori[1], np.eye(3).reshape(9))
        f = sw.fields(xs, ys)
        assert np.abs(f[0]).max() > 0 and np.abs(f[1]).max() > 0 and np.abs(f[0] - f[1]).max() > 1e-3 * np.abs(f[0]).max()
        for k in range(2):
            assert _same_bits(f[k], sw.single(k, xs, ys)), k
        c = pd_ref.solved_case(oracle, "earlier_segment")
        assert np.array_equal(sw.pos[0], c.position) and np.array_equal(sw.ori[0], c.orientation.reshape(9))
        scale = np.abs(c.oracle_field)
        live = scale > TAIL_FLOOR
        assert (np.abs(f[0] - c.oracle_field)[live] <= TAIL_ULPS * 2.0 ** -52 * scale[live]).all()
    finally:
        sw.close()


@pytest.mark.parametrize("name", ["earlier_segment", "three_segments", "child"])
def test_gauss_parameters_at_the_grids_z(oracle, solved, name):
    """bmo_gauss_parameters (gp_eval_kernel: the same pd_locate and gauss_parameters_at) against the oracle's gauss_parameters at the z of every
    grid point: the same doubles, NaNs included."""
    c, e = solved(name)
    rec = c.records[0]
    node = int(c.res.detector_nodes(c.slot)[0])
    z = pd_ref.restated_z(rec, c.position, c.orientation, c.xs, c.ys).reshape(-1)
    length = sum(s["t"] for s in rec["segs"]) + sum(t for chain in rec["parents"] for t, n in chain)
    l_parent = sum(t for chain in rec["parents"] for t, n in chain)
    if name == "child":
        assert 0.05 <= (z < l_parent).mean() <= 0.95
    else:
        assert 0.05 <= (z < length - rec["segs"][-1]["t"]).mean() <= 0.95  # part of the grid lies on an earlier segment
    a, b = c.osol.gauss_parameters(node, z), e.sol.gauss_parameters(node, z)
    assert np.isfinite(a).all() and (a[:, 0] > 0).all()
    assert np.array_equal(a, b, equal_nan=True), np.argwhere(a != b)[:5]
