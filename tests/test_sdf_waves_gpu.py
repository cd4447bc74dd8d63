"""The SDF step kernels on waves whose 64 lanes disagree (DESIGN.md §2 "SDF marches under incoherent waves").  tracing_step and sdf_any
(csrc/bmo_lane.hpp) take the union child evaluated first, the specialised march loop's child and the shape of every waterfall pass
from the wave's first active lane and walk the candidate slots by a scalar mask, while the nearest-hit prune, the start classification,
the retrace probe and the level boundary run on each lane's own state.  The host build of the lane code has one lane per wave.  Here
every wave mixes the eight ray families of tests/wave_scenes.py: forward, backward, from all around, starting on surfaces and in
glass, side-on, near misses and grazing rays, on four scenes.  Everything is bit for bit against the oracle, or between numberings of the
same rays; tests/test_sdf_waves.py checks on the CPU that the inputs are what this file assumes."""
import functools

import numpy as np
import pytest

import bmo_amd as bmo

from tests import wave_scenes as ws
from tests.parity import compare

pytestmark = pytest.mark.gpu
R_MAX = ws.R_MAX
N_KIND = 1024   # PolarizedRays and GaussianBeamlets
N_ORDER = 4096  # the numbering test: the smallest size at which the automatic root order sorts by chord


def _trace(monkeypatch, scene, bundle, order="none", env=None, wide=(None,)):
    """One solve per entry of `wide` (BMO_WIDE_MIN_WAVES, read per trace) with BMO_ROOT_ORDER = order (read when the batch is uploaded;
    None: unset) and `env` set before the engine is made; everything released again."""
    if order is None:
        monkeypatch.delenv("BMO_ROOT_ORDER", raising=False)
    else:
        monkeypatch.setenv("BMO_ROOT_ORDER", order)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = []
    eng = bmo.Engine(scene, 0)
    try:
        dev = eng.upload(bundle)
        try:
            for w in wide:
                if w is not None:
                    monkeypatch.setenv("BMO_WIDE_MIN_WAVES", w)
                res = eng.trace_device(dev, R_MAX)
                try:
                    out.append(eng.result_view(res))
                finally:
                    eng.free_result(res)
        finally:
            eng.free_batch(dev)
    finally:
        eng.close()
    return out


@functools.lru_cache(maxsize=None)
def _solved(name, kind="ray", n=ws.N_RAYS):
    """(scene, bundle, the oracle's solution) of a scene under its mixed bundle: computed once, shared, left unchanged."""
    import pyoracle

    system, parts, bundle, fam = ws.case(name, kind, n)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    return scene, bundle, pyoracle.trace(scene, bundle, R_MAX, threads=16)


CASES = [(name, "ray", ws.N_RAYS) for name in ws.SCENES] + [(name, kind, N_KIND) for name in ("c2", "train") for kind in ("pol", "gauss")]


@pytest.mark.parametrize("name,kind,n", CASES)
def test_mixed_waves(monkeypatch, name, kind, n):
    scene, bundle, ref = _solved(name, kind, n)
    assert bundle.n == n
    (got,) = _trace(monkeypatch, scene, bundle)
    compare(got, ref, 0.0, f"{name} {kind}, mixed waves")


@pytest.mark.parametrize("name", ["c2", "train"])
def test_mixed_waves_through_both_wave_builds(monkeypatch, name):
    """The step kernels compiled for 4 waves per SIMD (BMO_WIDE_MIN_WAVES=0) and for 3 (10^9)."""
    scene, bundle, ref = _solved(name)
    for w, got in zip(("0", "1000000000"), _trace(monkeypatch, scene, bundle, wide=("0", "1000000000"))):
        compare(got, ref, 0.0, f"{name}, BMO_WIDE_MIN_WAVES={w}")


VARIANTS = [{"BMO_FUSE": "1"}, {"BMO_FUSE": "3"}]  # (of tests/test_fuzz.py's VARIANTS; both wave builds: the test above)


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("name", ["c2", "train"])
def test_mixed_waves_kernel_variants(monkeypatch, name, env):
    scene, bundle, ref = _solved(name)
    (got,) = _trace(monkeypatch, scene, bundle, env=env)
    compare(got, ref, 0.0, f"{name}, {env}")


@pytest.mark.parametrize("name", ["c2", "train"])
def test_a_lanes_result_does_not_depend_on_its_wave(monkeypatch, name):
    """The same 4 096 rays numbered family after family (coherent waves), interleaved, and in a random order, and the interleaved
    numbering once more under the automatic root order (a chord sort at this size): every root's beam tree is the same bits, and the
    count of the reference's intersect3d calls is the same.  No oracle in the loop."""
    system, parts, bundle, fam = ws.case(name, "ray", N_ORDER)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    n = bundle.n
    orders = {"by family": ws.family_order(fam), "random": np.random.default_rng(20251105).permutation(n)}
    (base,) = _trace(monkeypatch, scene, bundle)
    trees = ws.by_root(base)
    assert base.n_nodes > n
    for label, order in orders.items():
        (got,) = _trace(monkeypatch, scene, ws.permuted(bundle, order))
        assert got.n_intersect_calls == base.n_intersect_calls, label
        assert got.n_nodes == base.n_nodes and got.n_records == base.n_records, label
        bad = ws.roots_differing(ws.by_root(got), trees, zip(range(n), order))
        assert bad == [], (name, label, len(bad), bad[:5], [ws.FAMILIES[fam[j]] for _, j in bad[:5]])
    (auto,) = _trace(monkeypatch, scene, bundle, order=None)
    compare(auto, base, 0.0, f"{name}, automatic root order against none")


def test_bad_lanes(monkeypatch, oracle):
    """Every 97th ray is NaN / Inf / zero / 1e30 m away, lane 0 (the lane readfirstlane reads) among them: engine equals oracle, and
    the good roots get what they get without bad neighbours."""
    scene, clean_bundle, _ = _solved("c2")
    bundle, bad = ws.bad_lanes(clean_bundle)
    ref = oracle.trace(scene, bundle, R_MAX, threads=16)
    (got,) = _trace(monkeypatch, scene, bundle)
    compare(got, ref, 0.0, "c2 with bad lanes")
    (clean,) = _trace(monkeypatch, scene, clean_bundle)
    good = np.flatnonzero(~bad)
    assert ws.roots_differing(ws.by_root(got), ws.by_root(clean), zip(good, good)) == []


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_partial_waves(monkeypatch, oracle, n):
    scene, bundle, _ = _solved("c2")
    part = ws.head(bundle, n)
    (got,) = _trace(monkeypatch, scene, part)
    compare(got, oracle.trace(scene, part, R_MAX, threads=16), 0.0, f"c2, {n} rays")


@pytest.mark.parametrize("kind,n", [("ray", ws.N_RAYS), ("gauss", N_KIND)])
def test_retrace_under_mixed_waves(monkeypatch, oracle, kind, n):
    """The first doublet moves by 0.05 mm and 0.3 deg: in one wave the probe of some lanes finds the stored path (their trees stay)
    and that of others misses (tests/test_sdf_waves.py counts both per wave).  The form of test_light_trap_retrace."""
    monkeypatch.setenv("BMO_ROOT_ORDER", "none")
    bundle = ws.case("c2", kind, n)[2]
    system = ws.fresh_system("c2")
    scene0 = bmo.CompiledScene(system, bundle.lambdas)
    a0, sol0 = oracle.trace(scene0, bundle, R_MAX, threads=16, keep=True)
    gs0 = gs1 = None
    try:
        g0, gs0 = bmo.system._engine_solve(scene0, bundle, R_MAX, None)
        compare(g0, a0, 0.0, f"c2 {kind}, fresh")
        ws.move_first_doublet(system)
        scene1 = bmo.CompiledScene(system, bundle.lambdas)
        a1 = oracle.trace(scene1, bundle, R_MAX, threads=16, prev=sol0)
        g1, gs1 = bmo.system._engine_solve(scene1, bundle, R_MAX, gs0)
        compare(g1, a1, 0.0, f"c2 {kind}, retrace after the doublet moved")
        assert not np.array_equal(a0.rec, a1.rec)
    finally:
        for s in (gs0, gs1, sol0):
            if s is not None:
                s.free()


def test_sweep_under_mixed_waves(monkeypatch, oracle):
    """Three positions of config 2's splitter in one solve_sweep, 1 024 mixed rays each: every configuration against the oracle's
    solve of its snapshot."""
    from test_sweep_gpu import _Slice

    monkeypatch.setenv("BMO_ROOT_ORDER", "none")
    n = N_KIND
    mixed = ws.case("c2", "ray", n)[2]
    system, parts = ws.SCENES["c2"][0]()
    beams = [bmo.Beam(bmo.Ray(mixed.planes[0:3, i], mixed.planes[3:6, i], ws.LAM)) for i in range(n)]
    bundle = bmo.RayBundle.from_beams(beams)  # (the Ray constructor normalises the directions once more: what the sweep traces)
    moves = [[0.0, 0.0, 0.0], [0.0, 0.2e-3, 0.5e-3], [0.1e-3, -0.3e-3, -0.4e-3]]

    def configure(c):
        bmo.translate3d(parts["bs"], moves[c])

    sol = bmo.solve_sweep(system, beams, 3, configure, r_max=R_MAX)
    try:
        calls = 0
        for c in range(3):
            ref = oracle.trace(sol.scenes[c], bundle, R_MAX, threads=16)
            sl = _Slice(sol.res, c, int(sol._node_start[c]), int(sol._node_start[c + 1]), c * n, n)
            sl.n_intersect_calls = ref.n_intersect_calls  # (a slice has no count of its own: the sum is compared below)
            calls += ref.n_intersect_calls
            compare(sl, ref, 0.0, f"c2 sweep, configuration {c}")
        assert sol.res.n_intersect_calls == calls
        assert not np.array_equal(sol.result(0).rec, sol.result(2).rec)  # the move changed the paths
    finally:
        sol.close()
