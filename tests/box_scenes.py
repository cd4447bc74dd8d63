"""Shared by tests/test_box_cull.py and tests/test_box_cull_gpu.py: host builds of the emulator with the box cull (csrc/bmo_lane.hpp
box_cull, DESIGN.md §3 "box cull") switched on and off, the box table of a compiled scene, and the directed mini scenes (64 rays or
fewer each) that aim at the cull's edge cases."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

import bmo_amd as bmo
from bmo_amd import abi
from scenes import disc_bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mm = 1e-3
LAM = 1.064e-6
R_MAX = 20
_libs = {}
_dir = None


def emu_dir():
    emu_lib(1)
    return _dir


def emu_lib(switch):
    """tests/emu/box_emu.cpp built with BMO_EMU_STATS and BMO_BOX_CULL = switch (fast path forced on, as the shipped Ray kernels have it)."""
    global _dir
    if switch not in _libs:
        if _dir is None:  # (BOX_EMU_BUILD_DIR: a test hands the directory of its builds to the child processes it starts)
            _dir = os.environ.get("BOX_EMU_BUILD_DIR") or tempfile.mkdtemp(prefix="bmo_box_emu_")
        so = os.path.join(_dir, "libbmo_box_emu_%d.so" % switch)
        if not os.path.exists(so):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-DBMO_EMU_STATS", "-DBMO_MARCH_FASTPATH=2",
                                   "-DBMO_BOX_CULL=%d" % switch, "-shared", "-o", so, os.path.join(ROOT, "tests", "emu", "box_emu.cpp")])
        L = C.CDLL(so)
        L.bmo_emu_trace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(C.c_void_p), C.POINTER(abi.ResultView)]
        L.bmo_emu_retrace.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.RayBatch), C.POINTER(abi.TraceOpts), C.POINTER(abi.ResultView),
                                      C.POINTER(C.c_void_p), C.POINTER(abi.ResultView)]
        L.bmo_emu_free.argtypes = [C.c_void_p]
        L.bmo_emu_box_counts.argtypes = [C.POINTER(C.c_long), C.c_int]
        L.bmo_emu_box_counts.restype = None
        L.bmo_emu_box_table.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        assert L.bmo_emu_box_switch() == switch
        _libs[switch] = L
    return _libs[switch]


def emu_trace(switch, scene, bundle, r_max=R_MAX, prev=None, max_beams=0):
    """parity.emu_trace through the library of emu_lib(switch); returns (TraceResult, marches started, candidates the box cull took)."""
    L = emu_lib(switch)
    batch, keep = bmo.make_batch(scene, bundle)
    o = abi.TraceOpts()
    o.r_max, o.device, o.record_segments, o.max_beams = int(r_max), 0, 1, int(max_beams)
    h, v = C.c_void_p(), abi.ResultView()
    counts = (C.c_long * 16)()
    L.bmo_emu_box_counts(counts, 1)
    if prev is None:
        rc = L.bmo_emu_trace(C.byref(scene.desc), C.byref(batch), C.byref(o), C.byref(h), C.byref(v))
    else:
        pv = prev.as_view()
        rc = L.bmo_emu_retrace(C.byref(scene.desc), C.byref(batch), C.byref(o), C.byref(pv), C.byref(h), C.byref(v))
    if rc == -6:
        raise RuntimeError("emulator: beam tree exceeds max_beams (-6)")
    assert rc == 0, rc
    try:
        res = abi.TraceResult(v)
    finally:
        L.bmo_emu_free(h)
    L.bmo_emu_box_counts(counts, 1)
    return res, int(counts[0]), int(counts[8])


def box_table(scene):
    """(table, raw): float64 [n_shapes, 6] = lo[3], hi[3] per shape id — the blob's table as the kernels read it, and the boxes before
    their margin.  lo > hi: the shape has no box."""
    n = scene.desc.n_shapes
    table, raw = np.zeros((n, 6)), np.zeros((n, 6))
    dp = C.POINTER(C.c_double)
    rc = emu_lib(1).bmo_emu_box_table(C.byref(scene.desc), table.ctypes.data_as(dp), raw.ctypes.data_as(dp))
    assert rc == 0, rc
    return table, raw


def hits_inside_boxes(scene, ref, tol=1e-9):
    """Every intersection point the result `ref` reports on a shape lies inside that shape's box before the margin, to `tol` metres.
    Returns the number of points checked (shapes without a box are not counted)."""
    _, raw = box_table(scene)
    rec, sid = np.asarray(ref.rec), np.asarray(ref.rec_shape)
    p, d, t = rec[0:3], rec[3:6], rec[7]  # (a GaussianBeamlet record: its chief ray, whose shape rec_shape is)
    ok = (sid >= 0) & np.isfinite(t)
    x = p[:, ok] + t[ok] * d[:, ok]
    lo, hi = raw[sid[ok], :3].T, raw[sid[ok], 3:].T
    has = lo[0] <= hi[0]
    assert ((x >= lo - tol) | ~has).all() and ((x <= hi + tol) | ~has).all(), "an intersection point outside its shape's box"
    return int(has.sum())


def _lens(y=0.0, d=12 * mm):
    lens = bmo.SphericalLens(30 * mm, -30 * mm, 5 * mm, d, 1.5)
    bmo.translate3d(lens, [0, y, 0])
    return lens


def _detector(y):
    det = bmo.Spotdetector(60 * mm)
    bmo.translate3d(det, [0, y, 0])
    return det


def _system(objs):
    """The objects plus a thin beam splitter parked behind the sources.  A scene with a splitter takes the engine's step kernels with
    in-loop splitters, and of the Ray kernels of the plain-shapes level it is that variant — in its build for large launches, which
    BMO_WIDE_MIN_WAVES=0 selects for any size — that runs the box test on the device (DESIGN.md §4 "Round 7")."""
    parked = bmo.ThinBeamsplitter(10 * mm)
    bmo.translate3d(parked, [0, -300 * mm, 0])
    return bmo.System(list(objs) + [parked])


def _rays(pos, dirs):
    pos, dirs = np.atleast_2d(np.asarray(pos, dtype=np.float64)), np.atleast_2d(np.asarray(dirs, dtype=np.float64))
    if dirs.shape[0] == 1:
        dirs = np.tile(dirs, (pos.shape[0], 1))
    return bmo.RayBundle.rays(pos, dirs, LAM)


def two_lenses():
    a, b = _lens(0.0), _lens(8 * mm)
    return _system([a, b, _detector(40 * mm)]), a, b


def face_plane_case(zeros):
    """Rays with `zeros` (1 or 2) zero direction components whose origins lie exactly on face planes of the first lens's box: on the
    front face they go on to hit the lens; on a side face (the axis of a zero component: the slab bounds would be 0 * inf) they pass by."""
    system, a, b = two_lenses()
    scene = bmo.CompiledScene(system, [LAM])
    lo, hi = np.split(box_table(scene)[0][scene.shape_id(a.shape)], 2)
    assert (lo < hi).all()
    d = [0.0, 1.0, 0.0] if zeros == 2 else [0.0, math.cos(0.05), math.sin(0.05)]
    pos = [[x, lo[1], z] for x in (0.0, 2 * mm, -4.5 * mm) for z in (0.0, 3 * mm)]  # front face plane: hits
    pos += [[lo[0], -10 * mm, 0.0], [hi[0], -10 * mm, 1 * mm], [lo[0], lo[1], 0.0], [hi[0], 2 * mm, 0.0]]  # side face planes of the zero x axis
    if zeros == 2:
        pos += [[0.0, -10 * mm, lo[2]], [lo[0], -10 * mm, hi[2]], [lo[0], lo[1], lo[2]]]  # ... and of the zero z axis, a box edge, a corner
    return scene, _rays(pos, d)


def rim_graze_case():
    """64 rays parallel to the axis across the rim of the first lens, 2 um to either side: inside the lens, inside the box's margin,
    outside the box (one wave whose lanes disagree on the cull of both lenses)."""
    system, a, b = two_lenses()
    x = 6 * mm + np.linspace(-2e-6, 2e-6, 64)
    pos = np.stack([x, np.full(64, -10 * mm), np.zeros(64)], axis=1)
    return bmo.CompiledScene(system, [LAM]), _rays(pos, [0.0, 1.0, 0.0])


def inside_box_case():
    """Origins inside the first lens's box — in the glass, and in the corners of the box outside the solid — in all directions."""
    system, a, b = two_lenses()
    scene = bmo.CompiledScene(system, [LAM])
    lo, hi = np.split(box_table(scene)[0][scene.shape_id(a.shape)], 2)
    rng = np.random.default_rng(3)
    pos = lo + (hi - lo) * rng.random((64, 3))
    dirs = rng.normal(size=(64, 3))
    return scene, _rays(pos, dirs / np.linalg.norm(dirs, axis=1)[:, None])


def tilted_case():
    """A lens tilted by 3 degrees and one tilted by 45 degrees behind it: their boxes are hulls of rotated corners."""
    a, b = _lens(0.0), _lens(14 * mm, 10 * mm)
    bmo.xrotate3d(a, math.radians(3))
    bmo.xrotate3d(b, math.radians(45))
    bmo.zrotate3d(b, math.radians(10))
    system = _system([a, b, _lens(30 * mm), _detector(50 * mm)])
    return bmo.CompiledScene(system, [LAM]), disc_bundle(64, [0, -10 * mm, 0], [0, 1, 0], 11 * mm, lam=LAM, seed=5, cone=0.3)


def mixed_union_case():
    """A union whose children have different rotations (a slab, a cylinder turned by 40 degrees about x, a sphere) in front of a lens."""
    slab, cyl, ball = bmo.BoxSDF(8 * mm, 2 * mm, 6 * mm), bmo.CylinderSDF(1.5 * mm, 4 * mm), bmo.SphereSDF(2 * mm)
    bmo.xrotate3d(cyl, math.radians(40))
    bmo.zrotate3d(cyl, math.radians(15))
    bmo.translate3d(cyl, [1 * mm, 1 * mm, 0])
    bmo.translate3d(ball, [-3 * mm, 2 * mm, 1 * mm])
    part = bmo.Lens(slab + cyl + ball, 1.5)
    bmo.zrotate3d(part, math.radians(-7))
    system = _system([part, _lens(12 * mm), _detector(40 * mm)])
    return bmo.CompiledScene(system, [LAM]), disc_bundle(64, [0, -10 * mm, 0], [0, 1, 0], 10 * mm, lam=LAM, seed=9, cone=0.2)


def no_box_case():
    """An asphere (an inexact shape: no box) and a lens whose description says bs_radius = -1 (no box either) between two plain lenses."""
    asph = bmo.Lens(bmo.EvenAsphericalSurface(40 * mm, 12 * mm, -0.8, [0.0, 1.0, 100.0]), bmo.SphericalSurface(-50 * mm, 12 * mm), 5 * mm, 1.5)
    bmo.translate3d(asph, [0, 8 * mm, 0])
    bare = _lens(16 * mm)
    system = _system([_lens(0.0), asph, bare, _lens(24 * mm), _detector(50 * mm)])
    scene = bmo.CompiledScene(system, [LAM])
    sid = scene.shape_id(bare.shape)
    scene._shapes[sid].bs_radius = -1.0
    table = box_table(scene)[0]
    assert table[sid, 0] > table[sid, 3] and table[scene.shape_id(asph.shape), 0] > table[scene.shape_id(asph.shape), 3]
    return scene, disc_bundle(64, [0, -10 * mm, 0], [0, 1, 0], 11 * mm, lam=LAM, seed=7, cone=0.15)


def plate_case():
    """A plate splitter (coating / substrate rule) behind lenses that are culled for the rays the plate sends sideways."""
    plate = bmo.RectangularPlateBeamsplitter(30 * mm, 30 * mm, 4 * mm, 1.5, reflectance=0.5)
    bmo.xrotate3d(plate, math.radians(45))
    bmo.translate3d(plate, [0, 25 * mm, 0])
    side = bmo.Spotdetector(60 * mm)
    bmo.xrotate3d(side, math.radians(90))
    bmo.translate3d(side, [0, 25 * mm, -50 * mm])
    system = bmo.System([_lens(0.0), _lens(8 * mm), plate, _lens(50 * mm), _detector(70 * mm), side])
    return bmo.CompiledScene(system, [LAM]), disc_bundle(48, [0, -10 * mm, 0], [0, 1, 0], 8 * mm, lam=LAM, seed=13, cone=0.05)


def rim_fan_case():
    """One wave whose lanes disagree: a 64-ray fan from one point across the rim of the first lens — the rays that pass outside it
    also miss the next lens's box, the others go through both."""
    system, a, b = two_lenses()
    x = np.linspace(4 * mm, 9 * mm, 64)
    dirs = np.stack([x, np.full(64, 10 * mm), np.zeros(64)], axis=1)
    return bmo.CompiledScene(system, [LAM]), _rays(np.tile([0.0, -10 * mm, 0.0], (64, 1)), dirs / np.linalg.norm(dirs, axis=1)[:, None])


DIRECTED = {
    "two_zero_components_on_face_planes": lambda: face_plane_case(2),
    "one_zero_component_on_face_planes": lambda: face_plane_case(1),
    "rim_graze_inside_the_margin": rim_graze_case,
    "origins_inside_the_box": inside_box_case,
    "lenses_tilted_3_and_45_degrees": tilted_case,
    "union_of_differently_rotated_children": mixed_union_case,
    "asphere_and_sphereless_lens_without_boxes": no_box_case,
    "plate_splitter_behind_culled_lenses": plate_case,
    "rim_fan_lanes_disagree": rim_fan_case,
}
