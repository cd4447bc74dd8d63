"""Mesh BVH on the GPU where the 64 lanes of a wave disagree (DESIGN.md §3 "mesh BVH"): mesh_nearest_bvh keeps one node stack per wave,
enters a child when any lane needs it, takes the child order and every popped node from the first active lane, and prunes with each lane's
own best hit and own limit.  Here every wave mixes the seven ray families of tests/mesh_scenes.py (hits and misses, all direction signs,
rays starting on faces and inside leaf boxes), holds non-finite lanes that leave for the brute-force loop, or is a partial wave; and in
the light trap lanes of one wave sit in different meshes of one node table, start on faces, and bring limits from another mesh's hit.
Everything is bit for bit against the oracle, which has no BVH.  tests/test_mesh_bvh_waves.py checks the inputs on the CPU."""
import functools
import math

import numpy as np
import pytest

import bmo_amd as bmo

from tests import mesh_scenes as ms
from tests.parity import compare

pytestmark = pytest.mark.gpu
mm = 1e-3
N = ms.DIRECTED_N
R_MAX = 5
TRAP_N = 4097
TRAP_R_MAX = 20


def _trace(monkeypatch, scene, bundle, order, r_max=R_MAX):
    """One solve with BMO_ROOT_ORDER = order (read when the batch is uploaded)."""
    monkeypatch.setenv("BMO_ROOT_ORDER", order)
    eng = bmo.Engine(scene, 0)
    try:
        dev = eng.upload(bundle)
        try:
            res = eng.trace_device(dev, r_max)
            try:
                return eng.result_view(res)
            finally:
                eng.free_result(res)
        finally:
            eng.free_batch(dev)
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def _directed(name):
    """(scene, bundle, the oracle's solution) of one mesh under its 14 337 interleaved rays."""
    import pyoracle

    v, f, bundle, _ = ms.directed_case(name)
    scene = ms.one_mesh_scene(v, f, bundle.lambdas)
    assert bmo.mesh_bvh_stats(scene)[0][0] > 0
    return scene, bundle, pyoracle.trace(scene, bundle, R_MAX, threads=16)


_clean = {}  # mesh name -> the engine's solution of the bundle without bad lanes, root order `none`


def _clean_solution(monkeypatch, name):
    if name not in _clean:
        scene, bundle, _ = _directed(name)
        _clean[name] = _trace(monkeypatch, scene, bundle, "none")
    return _clean[name]


@pytest.mark.parametrize("order", ["none", "auto"])
@pytest.mark.parametrize("name", list(ms.MESHES))
def test_directed_rays(monkeypatch, name, order):
    """`none` keeps the incoherent waves as built; `auto` (n >= 4096) sorts the roots by chord: the bundle's numbering and the same bits."""
    scene, bundle, ref = _directed(name)
    assert bundle.n == N
    got = _clean_solution(monkeypatch, name) if order == "none" else _trace(monkeypatch, scene, bundle, order)
    compare(got, ref, 0.0, f"{name}, root order {order}")


def _records_of(res, roots):
    """Indices of the records of the given roots' nodes (one node per root in these scenes)."""
    assert res.n_nodes == res.n_roots and np.array_equal(res.node_root, np.arange(res.n_roots))
    return np.concatenate([np.arange(a, a + n) for a, n in zip(res.node_first_rec[roots], res.node_nseg[roots])])


@pytest.mark.parametrize("name", ["sphere", "cuboid", "fan"])
def test_directed_rays_with_bad_lanes(oracle, monkeypatch, name):
    """Every 97th ray is NaN / Inf / zero / 1e30 away: such a lane runs the brute-force loop and returns while its wave goes on through
    the BVH (lane 0, the lane readfirstlane reads, among them).  The good lanes get what they get without bad neighbours."""
    scene, clean_bundle, _ = _directed(name)
    bundle, bad = ms.bad_lane_bundle(clean_bundle)
    ref = oracle.trace(scene, bundle, R_MAX, threads=16)
    got = _trace(monkeypatch, scene, bundle, "none")
    compare(got, ref, 0.0, f"{name} with bad lanes")
    clean = _clean_solution(monkeypatch, name)
    good = np.flatnonzero(~bad)
    for field in ("node_nseg", "node_status", "node_parent", "node_first_child"):
        assert np.array_equal(getattr(got, field)[good], getattr(clean, field)[good]), field
    rg, rc = _records_of(got, good), _records_of(clean, good)
    assert np.array_equal(got.rec_obj[rg], clean.rec_obj[rc]) and np.array_equal(got.rec_shape[rg], clean.rec_shape[rc])
    a, b = np.ascontiguousarray(got.rec[:, rg]), np.ascontiguousarray(clean.rec[:, rc])
    assert ((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_partial_waves(oracle, monkeypatch, n):
    scene, bundle, _ = _directed("sphere")
    part = bmo.RayBundle(bundle.kind, bundle.planes[:, :n].copy())
    compare(_trace(monkeypatch, scene, part, "none"), oracle.trace(scene, part, R_MAX, threads=16), 0.0, f"sphere, {n} rays")


def _trap(kind):
    system, parts = ms.light_trap_scene()
    bundle = ms.light_trap_bundle(kind, TRAP_N)
    return system, parts, bundle


@pytest.mark.parametrize("kind", ["ray", "pol", "gauss"])
def test_light_trap(oracle, kind):
    """Four BVHs in one node table and one mesh below the threshold; every bounce after the first starts on a face; the limit a lane
    brings to a mesh comes from another mesh's hit; every shell bounce is a tie between two coincident meshes."""
    system, parts, bundle = _trap(kind)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    assert sum(st[0] > 0 for st in bmo.mesh_bvh_stats(scene).values()) == 4
    ref = oracle.trace(scene, bundle, TRAP_R_MAX, threads=16)
    counts = [int((ref.rec_obj == i).sum()) for i in range(5)]
    assert all(c >= (1000 if kind == "ray" else 500) for c in counts[:4]) and counts[4] == 0, counts
    eng = bmo.Engine(scene, 0)
    try:
        got = eng.trace(bundle, TRAP_R_MAX)
    finally:
        eng.close()
    shell2 = next(i for i, o in enumerate(scene.leaf_objects) if o is parts["shell2"])
    assert shell2 == 4 and not np.any(got.rec_obj == shell2)
    compare(got, ref, 0.0, f"light trap, {kind}")


def test_light_trap_retrace(oracle):
    system, parts, bundle = _trap("ray")
    scene0 = bmo.CompiledScene(system, bundle.lambdas)
    a0, sol0 = oracle.trace(scene0, bundle, TRAP_R_MAX, threads=16, keep=True)
    g0, gs0 = bmo.system._engine_solve(scene0, bundle, TRAP_R_MAX, None)
    compare(g0, a0, 0.0, "light trap, fresh")
    bmo.translate3d(parts["ball"], [0.05 * mm, 0.1 * mm, 0])
    bmo.xrotate3d(parts["ball"], math.radians(0.3))
    scene1 = bmo.CompiledScene(system, bundle.lambdas)
    a1 = oracle.trace(scene1, bundle, TRAP_R_MAX, threads=16, prev=sol0)
    g1, gs1 = bmo.system._engine_solve(scene1, bundle, TRAP_R_MAX, gs0)
    compare(g1, a1, 0.0, "light trap, retrace after the ball moved")
    assert not np.array_equal(a0.rec, a1.rec)  # the move changed the paths
    for s in (gs0, gs1):
        s.free()
