"""Mesh BVH on the GPU (DESIGN.md §3 "mesh BVH"): the scenes H and M of tests/mesh_scenes.py traced through the BVH kernels (level 3)
against the oracle (brute force over every face, Mesh.jl:244-267) bit for bit — records, trees, detector data, n_intersect_calls — for
Ray, PolarizedRay and GaussianBeamlet, fresh and retraced after a move; the BVH engine against the brute-force engine
(mesh_bvh=False) at 2^18 rays; and a coarse speed check."""
import math

import numpy as np
import pytest

import bmo_amd as bmo

from tests import mesh_scenes as ms
from tests.parity import compare

mm = 1e-3
R_MAX = 20


def _make(name):
    if name == "H":
        system, parts = ms.housing_scene()
        return system, parts["housing"], lambda: bmo.translate3d(parts["system"].objects()[0], [0.05 * mm, 0, 0])
    system, parts = ms.mirror_scene()
    return system, parts["mirror"], lambda: bmo.xrotate3d(parts["mirror"], math.radians(0.3))


def _mesh_obj_index(scene, obj):
    return next(i for i, o in enumerate(scene.leaf_objects) if o is obj)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ray", "pol", "gauss"])
@pytest.mark.parametrize("name", ["H", "M"])
def test_gpu_mesh_scene_equals_oracle(oracle, name, kind):
    system, mesh_obj, move = _make(name)
    bundle = ms.bundle_of(kind, name, 4096)
    scene0 = bmo.CompiledScene(system, bundle.lambdas)
    assert any(st[0] > 0 for st in bmo.mesh_bvh_stats(scene0).values())
    a0, sol0 = oracle.trace(scene0, bundle, R_MAX, threads=16, keep=True)
    assert np.any(a0.rec_obj == _mesh_obj_index(scene0, mesh_obj)), "the mesh is never hit"
    if name == "M":
        assert int(a0.det_count.sum()) > 0
    g0, gs0 = bmo.system._engine_solve(scene0, bundle, R_MAX, None)
    compare(g0, a0, 0.0, f"{name}/{kind} fresh")
    move()
    scene1 = bmo.CompiledScene(system, bundle.lambdas)
    a1 = oracle.trace(scene1, bundle, R_MAX, threads=16, prev=sol0)
    g1, gs1 = bmo.system._engine_solve(scene1, bundle, R_MAX, gs0)
    compare(g1, a1, 0.0, f"{name}/{kind} retrace after a move")
    for s in (gs0, gs1):
        s.free()


def _trace(scene, bundle, reps=1):
    eng = bmo.Engine(scene, 0)
    try:
        out = [eng.trace(bundle, R_MAX) for _ in range(reps)]
    finally:
        eng.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["H", "M"])
def test_gpu_bvh_equals_brute_force_engine(name):
    system, _, _ = _make(name)
    bundle = ms.bundle_of("ray", name, 1 << 18)
    fast = _trace(bmo.CompiledScene(system, bundle.lambdas), bundle)[0]
    slow = _trace(bmo.CompiledScene(system, bundle.lambdas, mesh_bvh=False), bundle)[0]
    compare(fast, slow, 0.0, f"{name}: BVH against brute force")


@pytest.mark.gpu
def test_gpu_bvh_speed_on_mirror_scene():
    """Coarse: the BVH at least 5x faster than brute force on M (kernel time, best of 3 after a warm-up; loose, the machines are shared)."""
    system, _, _ = _make("M")
    bundle = ms.bundle_of("ray", "M", 1 << 18)
    fast = min(r.kernel_ms for r in _trace(bmo.CompiledScene(system, bundle.lambdas), bundle, 4)[1:])
    slow = min(r.kernel_ms for r in _trace(bmo.CompiledScene(system, bundle.lambdas, mesh_bvh=False), bundle, 4)[1:])
    print(f"\nM, 2^18 rays: BVH {fast:.3f} ms, brute force {slow:.3f} ms, x{slow / fast:.1f}")
    assert slow >= 5 * fast, (fast, slow)
