"""Mesh BVH (DESIGN.md §3 "mesh BVH"), CPU part: the builder's reports and the traversal against brute force, both through the
library's host entries on the scene blob the GPU reads (bmo_scene_mesh_bvh, bmo_mesh_nearest_host).  Brute force is the same entry on
the scene compiled with mesh_bvh=False (every face, Mesh.jl:244-267): t bits and face must agree for every ray."""
import ctypes as C
import time

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi

from tests import mesh_scenes as ms
from tests import scenes
from tests.mesh_scenes import MESHES, _cuboid_grid, _fan, _rays, _slivers, _soup, _sphere  # noqa: F401  (shared with test_mesh_bvh_waves*.py)

mm = 1e-3


def _scene(mesh, mesh_bvh=True):
    return bmo.CompiledScene(bmo.System([bmo.IntersectableObject(mesh)]), [1.064e-6], mesh_bvh=mesh_bvh)


def test_bvh_reported_for_large_mesh_only():
    v, f = ms.spherical_cap(0.1, 25 * mm, 50, 200)
    assert len(f) == 19800
    st = bmo.mesh_bvh_stats(_scene(bmo.Mesh(v, f)))
    n_nodes, depth, max_leaf = st[0]
    assert n_nodes > 2 * len(f) / 8 and 1 < depth <= 64 and 1 <= max_leaf <= 8, st
    assert bmo.mesh_bvh_stats(_scene(bmo.Mesh(v, f), mesh_bvh=False)) == {0: (0, 0, 0)}
    # just below / at the threshold
    small = bmo.CircularFlatMesh(10 * mm, bmo.shapes.MESH_BVH_MIN_FACES - 1)
    assert bmo.mesh_bvh_stats(_scene(small))[0][0] == 0
    assert bmo.mesh_bvh_stats(_scene(bmo.CircularFlatMesh(10 * mm, bmo.shapes.MESH_BVH_MIN_FACES)))[0][0] > 0


@pytest.mark.parametrize("make", [scenes.c1_scene, scenes.c2_scene, scenes.c4_scene, scenes.c5_scene])
def test_no_bvh_in_baseline_scenes(make):
    system, _ = make()
    st = bmo.mesh_bvh_stats(bmo.CompiledScene(system, [1.064e-6]))
    assert st and all(v == (0, 0, 0) for v in st.values()), st


def test_bvh_entries_reject_bad_arguments():
    lib = abi.load_engine()
    scene = _scene(bmo.CircularFlatMesh(10 * mm, 100))
    h = C.c_void_p()
    abi.check(lib, lib.bmo_scene_create(C.byref(scene.desc), C.byref(h)), "bmo_scene_create")
    try:
        n = C.c_int32()
        assert lib.bmo_scene_mesh_bvh(h, 1, C.byref(n), None, None) == -1
        assert lib.bmo_scene_mesh_bvh(h, -1, C.byref(n), None, None) == -1
        assert lib.bmo_scene_mesh_bvh(h, 0, C.byref(n), None, None) == 0 and n.value > 0
    finally:
        lib.bmo_scene_destroy(h)


def test_blob_over_4_gib_is_refused():
    """32-bit blob offsets: a scene whose tables would pass 4 GiB fails cleanly (before any triangle is read) instead of wrapping."""
    lib = abi.load_engine()
    scene = _scene(bmo.CircularFlatMesh(10 * mm, 100))
    d = scene.desc
    n_tris = d.n_tris
    d.n_tris = 60_000_000  # 72 B each: 4.3 GB
    h = C.c_void_p()
    try:
        rc = lib.bmo_scene_create(C.byref(d), C.byref(h))
    finally:
        d.n_tris = n_tris
    assert rc == -1
    assert b"4 GiB" in lib.bmo_last_error()


@pytest.mark.parametrize("name", list(MESHES))
def test_bvh_traversal_equals_brute_force(name):
    """10^6 rays over the five meshes: the BVH returns brute force's t bits and face for every one."""
    rng = np.random.default_rng(20251016)
    make, n = MESHES[name]
    v, f = make(rng)
    assert len(f) >= bmo.shapes.MESH_BVH_MIN_FACES
    mesh = bmo.Mesh(v, f)
    fast, slow = _scene(mesh), _scene(mesh, mesh_bvh=False)
    assert bmo.mesh_bvh_stats(fast)[0][0] > 0 and bmo.mesh_bvh_stats(slow)[0][0] == 0
    pos, dir = _rays(rng, v, f, n)
    t1, f1 = bmo.mesh_nearest_host(fast, 0, pos, dir)
    t0, f0 = bmo.mesh_nearest_host(slow, 0, pos, dir)
    bad = np.flatnonzero((t1.view(np.int64) != t0.view(np.int64)) | (f1 != f0))
    assert bad.size == 0, (name, bad[:5], t1[bad[:5]], t0[bad[:5]], f1[bad[:5]], f0[bad[:5]])
    hit = f0 >= 0
    assert 0.05 < hit.mean() < 1.0, hit.mean()  # (most slivers are thinner than kϵ allows: |Det| < kϵ for every ray)


def test_bvh_build_time_2e5_faces():
    v, f = ms.icosphere(6, 20 * mm)  # 81 920 faces per sphere
    v2 = np.concatenate([v, v + [50 * mm, 0, 0], v + [0, 50 * mm, 0]])
    f2 = np.concatenate([f, f + len(v), f + 2 * len(v)])[:200_000]
    mesh = bmo.Mesh(v2, f2)
    lib = abi.load_engine()
    scene = _scene(mesh)
    h = C.c_void_p()
    t = time.perf_counter()
    abi.check(lib, lib.bmo_scene_create(C.byref(scene.desc), C.byref(h)), "bmo_scene_create")
    dt = time.perf_counter() - t
    n, d, m = C.c_int32(), C.c_int32(), C.c_int32()
    lib.bmo_scene_mesh_bvh(h, 0, C.byref(n), C.byref(d), C.byref(m))
    lib.bmo_scene_destroy(h)
    print(f"\nbmo_scene_create with a BVH over {len(f2)} faces: {dt * 1e3:.1f} ms ({n.value} nodes, depth {d.value}, leaves <= {m.value})")
    assert n.value > 0
    assert dt < 5.0  # (target 0.2 s on one core: DESIGN.md §8; loose here, the machines are shared)
