"""Sweeps without a GPU: bmo_scene_create_sweep's topology rules and layout, bmo_trace_sweep's argument checks, solve_sweep's snapshots."""
import ctypes as C
import math

import numpy as np
import pytest

import bmo_amd as bmo
from bmo_amd import abi
from test_fuzz import random_system
from tests import mesh_scenes as ms
from tests.scenes import disc_bundle

mm = 1e-3
LAM = 1.064e-6


def _create(scenes):
    lib = abi.load_engine()
    descs = (abi.SceneDesc * len(scenes))(*[s.desc for s in scenes])
    h = C.c_void_p()
    rc = lib.bmo_scene_create_sweep(descs, len(scenes), C.byref(h))
    msg = lib.bmo_last_error().decode()
    return rc, h, msg, lib


def _snapshots(system, n, move):
    return bmo.sweep_snapshots(system, [LAM], n, move)[0]


def _mesh_system(level=2):
    v, f = ms.icosphere(level, 8 * mm)
    m = bmo.Mirror(bmo.Mesh(v, f))
    bmo.translate3d(m, [0, 40 * mm, 0])
    return m


def test_sweep_scene_accepts_moved_fuzz_snapshots_and_a_mesh_whose_bvh_changes():
    lib = abi.load_engine()
    for seed in (3, 11, 29):
        system = random_system(seed)[0]
        mesh = _mesh_system()
        system = bmo.System(list(system.objects()) + [mesh])
        rng = np.random.Generator(np.random.PCG64(seed))
        objs = list(system.objects())

        def move(c):
            for o in objs:
                bmo.translate3d(o, list(rng.uniform(-0.2, 0.2, 3) * mm))
            bmo.zrotate3d(mesh, math.radians(7.0 * c + 3.0))
            bmo.xrotate3d(mesh, math.radians(11.0 * c + 1.0))

        scenes = _snapshots(system, 6, move)
        sid = scenes[0].shape_id(mesh.shape)
        sizes = []
        for s in scenes:
            assert bmo.mesh_bvh_stats(s)[sid][0] > 0  # (n_nodes, depth, max_leaf): the mesh (320 faces) has a BVH
            sizes.append(bmo.mesh_bvh_stats(s)[sid][0])
        assert len(set(sizes)) > 1, sizes  # the rotated mesh's BVH changes size: the node table is sized to the largest
        rc, h, msg, _ = _create(scenes)
        assert rc == 0, msg
        # the handle describes configuration 0 where one configuration is asked for (bmo_scene_mesh_bvh)
        n = C.c_int32()
        d, m = C.c_int32(), C.c_int32()
        assert lib.bmo_scene_mesh_bvh(h, sid, C.byref(n), C.byref(d), C.byref(m)) == 0 and n.value == sizes[0]
        lib.bmo_scene_destroy(h)


def _refused(scenes, field):
    rc, h, msg, lib = _create(scenes)
    if rc == 0:
        lib.bmo_scene_destroy(h)
    assert rc == -1, (rc, msg)  # BMO_ERR_INVALID
    assert field in msg, msg


def test_sweep_scene_refuses_topology_changes():
    base = random_system(5)[0]
    objs = list(base.objects())
    s0 = bmo.CompiledScene(base, [LAM])
    # object count
    extra = bmo.RoundPlanoMirror(10 * mm, 2 * mm)
    bmo.translate3d(extra, [0, -50 * mm, 0])
    _refused([s0, bmo.CompiledScene(bmo.System(objs + [extra]), [LAM])], "n_objects")
    # object kind
    _refused([bmo.CompiledScene(bmo.System(objs + [bmo.Mirror(bmo.CylinderSDF(5 * mm, 2 * mm))]), [LAM]),
              bmo.CompiledScene(bmo.System(objs + [bmo.IntersectableObject(bmo.CylinderSDF(5 * mm, 2 * mm))]), [LAM])], "objects[%d].kind" % len(objs))
    # shape kind under the same object kind
    _refused([bmo.CompiledScene(bmo.System(objs + [bmo.Mirror(bmo.CylinderSDF(5 * mm, 2 * mm))]), [LAM]),
              bmo.CompiledScene(bmo.System(objs + [bmo.Mirror(bmo.BoxSDF(5 * mm, 2 * mm, 5 * mm))]), [LAM])], ".kind")
    # triangle count
    v1, f1 = ms.icosphere(1, 5 * mm)
    v2, f2 = ms.icosphere(2, 5 * mm)
    _refused([bmo.CompiledScene(bmo.System(objs + [bmo.Mirror(bmo.Mesh(v1, f1))]), [LAM]),
              bmo.CompiledScene(bmo.System(objs + [bmo.Mirror(bmo.Mesh(v2, f2))]), [LAM])], "n_tris")
    # wavelengths
    _refused([s0, bmo.CompiledScene(base, [LAM * 1.5])], "lambdas")
    _refused([s0, bmo.CompiledScene(base, [LAM, LAM * 1.5])], "n_lambda")
    # tracing constants
    _refused([s0, bmo.CompiledScene(base, [LAM], consts=dict(eps_srf=2e-9))], "eps_srf")
    _refused([s0, bmo.CompiledScene(base, [LAM], consts=dict(march_iters=500))], "march_iters")
    # and the same snapshot twice is fine
    rc, h, msg, lib = _create([s0, bmo.CompiledScene(base, [LAM])])
    assert rc == 0, msg
    lib.bmo_scene_destroy(h)


def test_existing_entries_refuse_a_sweep_scene():
    base = random_system(7)[0]
    s0 = bmo.CompiledScene(base, [LAM])
    rc, h, msg, lib = _create([s0, s0])
    assert rc == 0, msg
    try:
        bundle = disc_bundle(16, center=[0, -5 * mm, 0], direction=[0, 1, 0], diameter=2 * mm, lam=LAM)
        batch, keep = bmo.make_batch(s0, bundle)
        o = abi.TraceOpts()
        o.r_max, o.device, o.record_segments, o.max_beams = 100, 0, 1, 0
        res = C.c_void_p()
        assert lib.bmo_trace(h, C.byref(batch), C.byref(o), C.byref(res)) == -1
        assert "bmo_trace_sweep" in lib.bmo_last_error().decode()
        b = C.c_void_p()
        assert lib.bmo_batch_upload(h, C.byref(batch), 0, C.byref(b)) == -1
    finally:
        lib.bmo_scene_destroy(h)


def test_trace_sweep_checks_root_config_before_the_device():
    base = random_system(9)[0]
    scenes = [bmo.CompiledScene(base, [LAM]) for _ in range(3)]
    rc, h, msg, lib = _create(scenes)
    assert rc == 0, msg
    try:
        bundle = disc_bundle(6, center=[0, -5 * mm, 0], direction=[0, 1, 0], diameter=2 * mm, lam=LAM)
        batch, keep = bmo.make_batch(scenes[0], bundle)
        o = abi.TraceOpts()
        o.r_max, o.device, o.record_segments, o.max_beams = 100, 0, 1, 0
        res = C.c_void_p()
        for bad, what in (([0, 0, 2, 1, 2, 2], "decreases"), ([0, 0, 1, 1, 2, 3], "not in [0, 3)"), ([-1, 0, 0, 1, 1, 2], "not in [0, 3)")):
            cfg = np.array(bad, dtype=np.int32)
            assert lib.bmo_trace_sweep(h, C.byref(batch), cfg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(o), C.byref(res)) == -1
            assert what in lib.bmo_last_error().decode()
        good = np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)
        rc = lib.bmo_trace_sweep(h, C.byref(batch), good.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(o), C.byref(res))
        if lib.bmo_device_count() == 0:
            assert rc == -2, lib.bmo_last_error().decode()  # no GPU: a loud BMO_ERR_NO_DEVICE, no fallback
        else:
            assert rc == 0, lib.bmo_last_error().decode()
            lib.bmo_result_free(res)
        # an ordinary scene is not a sweep
        plain = C.c_void_p()
        assert lib.bmo_scene_create(C.byref(scenes[0].desc), C.byref(plain)) == 0
        assert lib.bmo_trace_sweep(plain, C.byref(batch), good.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(o), C.byref(res)) == -1
        lib.bmo_scene_destroy(plain)
    finally:
        lib.bmo_scene_destroy(h)


def test_sweep_snapshots_call_configure_in_order_and_keep_their_numbers():
    m = bmo.RoundPlanoMirror(20 * mm, 3 * mm)
    pd = bmo.Photodetector(5 * mm, 8)
    bmo.translate3d(pd, [0, 50 * mm, 0])
    system = bmo.System([m, pd])
    calls = []

    def configure(c):
        calls.append(c)
        bmo.translate_to3d(m, [0, (10 + c) * mm, 0])
        bmo.translate_to3d(pd, [0, (50 + 2 * c) * mm, 0])

    scenes, poses, grids = bmo.sweep_snapshots(system, [LAM], 4, configure)
    assert calls == [0, 1, 2, 3]
    sid = scenes[0].shape_id(m.shape)
    for c, s in enumerate(scenes):
        assert s._shapes[sid].pos[1] == (10 + c) * mm  # later configure calls moved the same mirror: the snapshot kept its numbers
        assert poses[c][0][0][1] == (50 + 2 * c) * mm
    assert np.array_equal(grids[0][0], pd.x)
    # the system is left as the last configure call made it
    assert m.position()[1] == 13 * mm

    def bad(c):
        if c == 2:
            pd.resolution(10)

    with pytest.raises(ValueError, match="resolution"):
        bmo.sweep_snapshots(system, [LAM], 3, bad)
