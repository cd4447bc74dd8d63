"""The cases of the state-independence tests (not a test file): every C entry that touches the device, run at the smallest shapes that
still have the structure that goes wrong, returning everything the entry writes as a dict of arrays.

A case is a function without required arguments; `entries` names the C entries of include/bmo.h it reaches and `group` the child process
of tests/test_state_independence_gpu.py that runs it under BMO_POOL_POISON.  tests/test_state_cases.py holds the union of the `entries`
to the header: a read-out added later without a case fails there.

What a case returns must depend on nothing but its inputs: not on what the pools' recycled blocks hold (DESIGN.md §2 "State
independence"), not on what the caller's output buffers hold, not on the calls that ran before it.  The inputs of the read-outs that take
rows are rows of the oracle (a CPU trace) or of a seeded generator, so a read-out case tests the read-out alone.

Shapes of the read-outs that take rows: H = 0 (no rows), 257 (one LDS tile and a row) and 5000 (twenty splits of one LDS tile with a ragged
last on these small grids, readout_ref.psf_splits; three row splits with a ragged third in the statistic passes, spot_ref.spot_splits), and an H = 300 call of the same entry immediately before
the H = 257 one: 300 rows are 21 600 B <= 1.25 * 18 504 B + 4 096 B, so the second call's row buffer is the first call's larger block.
The sweep forms read a three-configuration sweep whose middle configuration has no roots, at a pose per configuration.

Arguments an entry both reads and writes are handed zeros by the case itself, never the sentinel:
  bmo_photodetector_field        field_inout (include/bmo.h:428, "contributions are ADDED")
  bmo_photodetector_field_sweep  field_inout (include/bmo.h:478, "contributions ADDED")
"""
import ctypes as C
import functools
import math
import re
import os

import numpy as np

import bmo_amd as bmo
import poly_ref as pr
import readout_ref as rr
import scenes
import spot_ref as sr
from bmo_amd import abi
from bmo_amd.system import _engine_solve
from test_photodetector import pd_scene
from test_retrace import retrace_pair
from test_splitter_chain import _bundle as chain_bundle, _chain

mm = 1e-3
R_MAX = 20
ROW_COUNTS = (0, 300, 257, 5000)  # (300 right before 257: the recycled larger block)
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bmo.h")

CASES = []
GROUPS = ("trace", "psf", "wavefront", "focus", "spot_pd", "poly")


def case(group, *entries):
    def deco(f):
        assert group in GROUPS
        f.group, f.entries, f.name = group, tuple(entries), f.__name__
        CASES.append(f)
        return f

    return deco


def header_entries():
    """The C entries include/bmo.h declares."""
    text = open(HEADER, encoding="utf-8").read()
    return set(re.findall(r"^(?:int|double|const char\*)\s+(bmo_[a-z0-9_]+)\(", text, re.M))


# Entries no case reaches, each with its reason.
EXCLUDED = {
    "bmo_version": "a constant: no device, no buffer",
    "bmo_source_hash": "a constant string: no device, no buffer",
    "bmo_build_flags_hash": "a constant string: no device, no buffer",
    "bmo_last_error": "the thread's error text: no device, no buffer",
    "bmo_device_count": "asks the runtime: no buffer",
    "bmo_jl_trig": "host only: the host build of bmo_jlmath.hpp, one value in, one out",
    "bmo_scene_mesh_bvh": "host only: describes the BVH built at bmo_scene_create",
    "bmo_mesh_nearest_host": "host only: the lane code's mesh intersection compiled for the host",
    "bmo_result_timing": "timing: differs from run to run by nature",
    "bmo_pool_release": "the tests' own tool: frees the pool, writes nothing",
    "bmo_scene_destroy": "destroy: frees, writes nothing",
    "bmo_batch_free": "free: writes nothing",
    "bmo_result_free": "free: writes nothing",
    "bmo_psf_bands_free": "free: writes nothing",
}


# ------------------------------------------------------------------------------------------------ results as dicts of arrays
_TRACE_FIELDS = ("node_root", "node_parent", "node_first_child", "node_first_rec", "node_nseg", "node_status", "node_aux", "rec_obj", "rec_shape", "rec",
                 "det_count", "det_offset", "det_node", "det_data")


def trace_dict(res, prefix=""):
    """Everything of an abi.TraceResult (a host copy of a whole result view) but its timing."""
    out = {prefix + name: getattr(res, name) for name in _TRACE_FIELDS}
    out[prefix + "counts"] = np.array([res.n_roots, res.n_nodes, res.n_records, res.n_intersect_calls, res.n_steps, res.beam_kind, res.rec_planes,
                                       res.n_detectors], dtype=np.int64)
    return out


def _put(out, prefix, names, values):
    """values (a wrapper's return tuple without its kernel_ms) under prefix + name; None (an output not asked for) is left out"""
    for name, v in zip(names, values):
        if v is not None:
            out[prefix + name] = np.asarray(v)


# ------------------------------------------------------------------------------------------------ the trace cases
def _splitter_trace(kind, keep):
    """Ray / PolarizedRay / GaussianBeamlet through a lens, two thin splitters and a Spotdetector, 96 roots, the segment log kept and the
    whole result view read."""
    bundle = chain_bundle(kind, 96)
    scene = bmo.CompiledScene(_chain(2), bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    try:
        res = eng.trace(bundle, 50)
    finally:
        eng.close()
    if keep is not None:
        keep.append((kind, res, scene, bundle, 50, None))
    return trace_dict(res)


@case("trace", "bmo_scene_create", "bmo_trace", "bmo_result_view")
def trace_ray(keep=None):
    return _splitter_trace("ray", keep)


@case("trace", "bmo_scene_create", "bmo_trace", "bmo_result_view")
def trace_polarized(keep=None):
    return _splitter_trace("pol", keep)


@case("trace", "bmo_scene_create", "bmo_trace", "bmo_result_view")
def trace_gaussian(keep=None):
    return _splitter_trace("gauss", keep)


@case("trace", "bmo_scene_create", "bmo_batch_upload", "bmo_trace_device", "bmo_result_view_select", "bmo_result_counts", "bmo_result_device_hits",
      "bmo_result_copy_hits", "bmo_result_copy_hit_columns", "bmo_result_view")
def trace_device_views():
    """A detector-only solve (record_segments = 0) and a solve with the log of one uploaded batch; the selective views (hits alone, the last
    segment, then the whole log), the counts, and the hit copies into host memory."""
    bundle = chain_bundle("ray", 96)
    scene = bmo.CompiledScene(_chain(2), bundle.lambdas)
    eng = bmo.Engine(scene, 0)
    out = {}
    try:
        batch = eng.upload(bundle)
        try:
            for label, log in (("nolog/", False), ("log/", True)):
                h = eng.trace_device(batch, 50, record_segments=log)
                try:
                    out[label + "size"] = np.array(eng.result_size(h), dtype=np.int64)
                    out.update(trace_dict(eng.result_view(h, abi.VIEW_HITS), label + "hits/"))
                    if log:
                        out.update(trace_dict(eng.result_view(h, abi.VIEW_HITS | abi.VIEW_LAST_SEGMENT), label + "last/"))
                        out.update(trace_dict(eng.result_view(h), label + "all/"))
                    else:
                        out.update(trace_dict(eng.result_view(h), label + "all/"))
                    slot = 0
                    _, cnt = eng.result_device_hits(h, slot)
                    out[label + "count"] = np.array([cnt], dtype=np.int64)
                    full, cols = abi._out((cnt, 9)), abi._out((cnt, 2))
                    eng.result_copy_hits(h, slot, full.ctypes.data, cnt)
                    eng.result_copy_hit_columns(h, slot, 2, cols.ctypes.data, cnt)
                    out[label + "copy_hits"], out[label + "copy_hit_columns"] = full, cols
                finally:
                    eng.free_result(h)
        finally:
            eng.free_batch(batch)
    finally:
        eng.close()
    return out


@case("trace", "bmo_scene_create", "bmo_trace", "bmo_retrace", "bmo_result_view")
def retrace_after_a_move(keep=None):
    """bmo_retrace of a solved Ray and a solved GaussianBeamlet batch after a kinematic move (a tilted splitter), and back."""
    out = {}
    for kind in ("ray", "gauss"):
        scene0, scene1, bundle = retrace_pair(kind, "tilt_splitter", 96)
        g0, s0 = _engine_solve(scene0, bundle, R_MAX, None)
        g1, s1 = _engine_solve(scene1, bundle, R_MAX, s0)
        g2, s2 = _engine_solve(scene0, bundle, R_MAX, s1)
        for s in (s0, s1, s2):
            s.free()
        if keep is not None:
            keep.append((kind + " first", g0, scene0, bundle, R_MAX, None))
            keep.append((kind + " retrace", g1, scene1, bundle, R_MAX, (scene0,)))
        for label, g in (("first/", g0), ("retrace/", g1), ("back/", g2)):
            out.update(trace_dict(g, kind + "/" + label))
    return out


@case("trace", "bmo_scene_create", "bmo_batch_upload", "bmo_trace_device", "bmo_retrace_device", "bmo_result_view")
def retrace_device_after_a_move(keep=None):
    """bmo_retrace_device on a resident batch: the scene moved (a lens shifted sideways: stored hits are lost, beams cut and traced on)."""
    scene0, scene1, bundle = retrace_pair("ray", "shift_train", 96)
    out = {}
    e0, e1 = bmo.Engine(scene0, 0), bmo.Engine(scene1, 0)
    try:
        batch = e0.upload(bundle)
        h0 = e0.trace_device(batch, R_MAX)
        h1 = e1.retrace_device(batch, h0, R_MAX)
        v0, v1 = e0.result_view(h0), e1.result_view(h1)
        if keep is not None:
            keep.append(("first", v0, scene0, bundle, R_MAX, None))
            keep.append(("retrace", v1, scene1, bundle, R_MAX, (scene0,)))
        out.update(trace_dict(v0, "first/"))
        out.update(trace_dict(v1, "retrace/"))
        e1.free_result(h1)
        e0.free_result(h0)
        e0.free_batch(batch)
    finally:
        e0.close()
        e1.close()
    return out


def _root_config(n0, n2):
    """roots of a three-configuration sweep whose middle configuration is empty"""
    return np.concatenate([np.zeros(n0, dtype=np.int32), np.full(n2, 2, dtype=np.int32)])


@case("trace", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_result_view")
def trace_sweep():
    """bmo_trace_sweep with K = 3 and one empty configuration, for Ray and GaussianBeamlet roots through the splitters."""
    out = {}
    for kind in ("ray", "gauss"):
        bundle = chain_bundle(kind, 96)
        system = _chain(2)
        objs = list(system.objects())

        def configure(c):
            bmo.translate3d(objs[0], [0.05 * mm * c, 0, 0.02 * mm * c])

        snaps = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)[0]
        res, h, lib = bmo.sweep_trace(snaps, bundle, _root_config(40, 56), 50, 0, True)
        lib.bmo_result_free(h)
        out.update(trace_dict(res, kind + "/"))
    return out


# ------------------------------------------------------------------------------------------------ PSF rows and the PSF sweep
@functools.lru_cache(maxsize=None)
def _psf_setup():
    """The tilted PSF scene of readout_ref with 5 000 rays: (rows [5000, 9] of the oracle, origin, e1, e2, normal)."""
    import pyoracle

    system, psfd, bundle = rr.tilted_psf_case(5000)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    slot = next(i for i, d in enumerate(scene.detectors) if d is psfd)
    rows = np.ascontiguousarray(pyoracle.trace(scene, bundle, 100, threads=8).detector_hits(slot))
    assert len(rows) == 5000, len(rows)
    ori = np.array(psfd.orientation(), dtype=np.float64)
    return rows, np.array(psfd.position(), dtype=np.float64), ori[:, 0].copy(), ori[:, 2].copy(), ori[:, 1].copy()


def _axes(n, half=30e-6):
    return np.linspace(-half, half, n), np.linspace(-0.8 * half, 1.1 * half, n)


class _PsfSweep:
    """A three-configuration sweep of the tilted PSF scene, the detector at another pose in each, the middle one without roots: the result
    handle with 300 rows in configuration 0 and 257 in configuration 2."""

    K = 3

    def __enter__(self):
        system, psfd, bundle = rr.tilted_psf_case(557)
        p0 = np.array(psfd.position(), dtype=np.float64)

        def configure(c):
            bmo.translate_to3d(psfd, list(p0 + np.array([0.01 * mm * c, 0.05 * mm * c, -0.02 * mm * c])))
            bmo.xrotate3d(psfd, math.radians(0.3 * c))

        snaps, poses, _ = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)
        self.slot = next(i for i, d in enumerate(snaps[0].detectors) if d is psfd)
        _, self.handle, self.lib = bmo.sweep_trace(snaps, bundle, _root_config(300, 257), 100, 0, True, view=False)
        self.pos = np.ascontiguousarray([poses[c][self.slot][0] for c in range(3)], dtype=np.float64)
        ori = np.ascontiguousarray([poses[c][self.slot][1] for c in range(3)], dtype=np.float64)
        self.e1, self.e2 = np.ascontiguousarray(ori[:, :, 0]), np.ascontiguousarray(ori[:, :, 2])
        return self

    def __exit__(self, *exc):
        self.lib.bmo_result_free(self.handle)


def _per_rows(f):
    """f(rows) -> dict, for every row count of ROW_COUNTS in that order, under "H<count>/"."""
    rows = _psf_setup()[0]
    out = {}
    for H in ROW_COUNTS:
        for k, v in f(rows[:H]).items():
            out["H%d/%s" % (H, k)] = v
    return out


@case("psf", "bmo_psf_intensity")
def psf_intensity():
    _, o, e1, e2, _ = _psf_setup()
    xs, zs = _axes(8)

    def f(rows):
        d = {}
        _put(d, "field/", ("I", "F"), abi.psf_intensity(rows, o, e1, e2, xs, zs, want_field=True)[:2])
        _put(d, "plain/", ("I", "F"), abi.psf_intensity(rows, o, e1, e2, xs, zs)[:2])
        return d

    return _per_rows(f)


@case("psf", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_psf_intensity_sweep")
def psf_intensity_sweep():
    xs, zs = _axes(8)
    out = {}
    with _PsfSweep() as sw:
        ax, az = np.tile(xs, (3, 1)) + 1e-6 * np.arange(3)[:, None], np.tile(zs, (3, 1))
        _put(out, "field/", ("I", "F"), abi.psf_intensity_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, ax, az, want_field=True)[:2])
        _put(out, "plain/", ("I", "F"), abi.psf_intensity_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, ax, az)[:2])
    return out


@case("psf", "bmo_psf_stats")
def psf_stats():
    _, o, e1, e2, _ = _psf_setup()

    def f(rows):
        return {"centroid": abi.psf_stats(rows, o, e1, e2)[0], "ref": abi.psf_stats(rows, o, e1, e2, ref=(1e-5, -2e-5))[0]}

    return _per_rows(f)


@case("psf", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_psf_stats_sweep")
def psf_stats_sweep():
    with _PsfSweep() as sw:
        return {"centroid": abi.psf_stats_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2)[0],
                "ref": abi.psf_stats_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, ref=[(0, 0), (1e-5, 0), (0, -1e-5)])[0]}


@case("psf", "bmo_scene_create", "bmo_batch_upload", "bmo_trace_device", "bmo_result_psf_rows", "bmo_psf_stats", "bmo_psf_stats_sweep", "bmo_psf_intensity")
def psf_resident_rows():
    """The rows of an ordinary (non-sweep) detector-only solve where they lie: bmo_result_psf_rows hands their device pointer to the single
    calls, and the sweep form reads them as its one configuration."""
    system, psfd, bundle = rr.tilted_psf_case(300)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    slot = next(i for i, d in enumerate(scene.detectors) if d is psfd)
    o, ori = np.array(psfd.position(), dtype=np.float64), np.array(psfd.orientation(), dtype=np.float64)
    e1, e2 = ori[:, 0].copy(), ori[:, 2].copy()
    xs, zs = _axes(8)
    eng = bmo.Engine(scene, 0)
    out = {}
    try:
        batch = eng.upload(bundle)
        h = eng.trace_device(batch, 100, record_segments=False)
        try:
            p, cnt, dev = C.POINTER(C.c_double)(), C.c_int64(), C.c_int32()
            abi.check(eng.lib, eng.lib.bmo_result_psf_rows(h, slot, C.byref(p), C.byref(cnt), C.byref(dev)), "bmo_result_psf_rows")
            ptr = C.cast(p, C.c_void_p).value or 0
            out["count_device"] = np.array([cnt.value, dev.value], dtype=np.int64)
            out["stats"] = abi.psf_stats(None, o, e1, e2, device=dev.value, hits_device_ptr=ptr, n_hits=cnt.value)[0]
            out["stats_as_one_configuration"] = abi.psf_stats_sweep(h, slot, 1, o, e1, e2)[0]
            _put(out, "", ("I", "F"), abi.psf_intensity(None, o, e1, e2, xs, zs, device=dev.value, hits_device_ptr=ptr, n_hits=cnt.value, want_field=True)[:2])
        finally:
            eng.free_result(h)
            eng.free_batch(batch)
    finally:
        eng.close()
    return out


# ------------------------------------------------------------------------------------------------ wavefront: Zernike fit and OPD map
ZORDER = 6


def _finite(a):
    return np.nan_to_num(np.asarray(a, dtype=np.float64), nan=0.0, posinf=0.0, neginf=0.0)


@case("wavefront", "bmo_psf_zernike")
def psf_zernike():
    _, o, e1, e2, _ = _psf_setup()

    def f(rows):
        d = {}
        _put(d, "", ("coef", "info", "gram"), abi.psf_zernike(rows, o, e1, e2, order=ZORDER, want_gram=True)[:3])
        _put(d, "nogram/", ("coef", "info", "gram"), abi.psf_zernike(rows, o, e1, e2, order=ZORDER)[:3])
        return d

    return _per_rows(f)


@case("wavefront", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_psf_zernike_sweep")
def psf_zernike_sweep():
    out = {}
    with _PsfSweep() as sw:
        _put(out, "", ("coef", "info", "gram"), abi.psf_zernike_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, order=ZORDER, want_gram=True)[:3])
        _put(out, "nogram/", ("coef", "info", "gram"), abi.psf_zernike_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, order=ZORDER)[:3])
    return out


_OPD = ("opd", "weight", "count", "info", "raw")


@case("wavefront", "bmo_psf_zernike", "bmo_psf_opd_map")
def psf_opd_map():
    """n = 8 bins, the fitted surface removed (remove = "fit": the coefficients of bmo_psf_zernike handed back), with the raw sums."""
    _, o, e1, e2, _ = _psf_setup()

    def f(rows):
        coef = _finite(abi.psf_zernike(rows, o, e1, e2, order=ZORDER)[0])  # (no rows: a NaN fit; zeros then)
        d = {}
        _put(d, "fit/", _OPD, abi.psf_opd_map(rows, o, e1, e2, n=8, order=ZORDER, coef=coef, want_raw=True)[:5])
        _put(d, "none/", _OPD, abi.psf_opd_map(rows, o, e1, e2, n=8)[:5])
        return d

    return _per_rows(f)


@case("wavefront", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_psf_zernike_sweep", "bmo_psf_opd_map_sweep")
def psf_opd_map_sweep():
    out = {}
    with _PsfSweep() as sw:
        coef = _finite(abi.psf_zernike_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, order=ZORDER)[0])
        _put(out, "fit/", _OPD, abi.psf_opd_map_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, n=8, order=ZORDER, coef=coef, want_raw=True)[:5])
        _put(out, "none/", _OPD, abi.psf_opd_map_sweep(sw.handle, sw.slot, 3, sw.pos, sw.e1, sw.e2, n=8)[:5])
    return out


# ------------------------------------------------------------------------------------------------ through focus, MTF, encircled energy
M_PLANES = 17


def _planes():
    normal = _psf_setup()[4]
    off = np.linspace(-1 * mm, 1 * mm, M_PLANES)
    return off, off[:, None] * normal[None, :]


FREQS = np.array([[0.0, 0.0], [2e3, 0.0], [0.0, 3e3], [5e3, -4e3], [1e4, 1e4]])
RADII = np.array([5e-6, 1e-6, 2e-5, 1e-4])


@case("focus", "bmo_psf_through_focus")
def psf_through_focus():
    _, o, e1, e2, _ = _psf_setup()
    xs, zs = _axes(5)
    _, disp = _planes()

    def f(rows):
        d = {}
        _put(d, "field/", ("I", "F"), abi.psf_through_focus(rows, o, e1, e2, disp, xs, zs, want_field=True)[:2])
        _put(d, "plain/", ("I", "F"), abi.psf_through_focus(rows, o, e1, e2, disp, xs, zs)[:2])
        return d

    return _per_rows(f)


@case("focus", "bmo_psf_focus_stats")
def psf_focus_stats():
    _, o, e1, e2, normal = _psf_setup()
    off, _ = _planes()
    return _per_rows(lambda rows: {"stats": abi.psf_focus_stats(rows, o, e1, e2, normal, off)[0]})


@case("focus", "bmo_psf_geo_otf")
def psf_geo_otf():
    _, o, e1, e2, normal = _psf_setup()
    off, _ = _planes()
    cen = np.stack([1e-6 * np.arange(M_PLANES), -2e-6 * np.arange(M_PLANES)], axis=1)

    def f(rows):
        d = {}
        _put(d, "origin/", ("mtf", "otf", "sums"), abi.psf_geo_otf(rows, o, e1, e2, normal, off, FREQS)[:3])
        _put(d, "centers/", ("mtf", "otf", "sums"), abi.psf_geo_otf(rows, o, e1, e2, normal, off, FREQS, centers=cen)[:3])
        return d

    return _per_rows(f)


@case("focus", "bmo_psf_otf")
def psf_otf():
    _, o, e1, e2, _ = _psf_setup()
    xs, zs = _axes(5)
    _, disp = _planes()

    def f(rows):
        d = {}
        _put(d, "image/", ("mtf", "otf", "sums", "I"), abi.psf_otf(rows, o, e1, e2, disp, xs, zs, FREQS, want_intensity=True)[:4])
        _put(d, "plain/", ("mtf", "otf", "sums", "I"), abi.psf_otf(rows, o, e1, e2, disp, xs, zs, FREQS)[:4])
        return d

    return _per_rows(f)


@case("focus", "bmo_psf_geo_ee")
def psf_geo_ee():
    _, o, e1, e2, normal = _psf_setup()
    off, _ = _planes()

    def f(rows):
        d = {}
        for shape in ("circle", "square"):
            _put(d, shape + "/", ("ee", "energy", "count", "sums"), abi.psf_geo_ee(rows, o, e1, e2, normal, off, RADII, shape=shape, want_count=True)[:4])
        _put(d, "nocount/", ("ee", "energy", "count", "sums"), abi.psf_geo_ee(rows, o, e1, e2, normal, off, RADII, want_count=False)[:4])
        return d

    return _per_rows(f)


@case("focus", "bmo_psf_ee")
def psf_ee():
    _, o, e1, e2, _ = _psf_setup()
    xs, zs = _axes(5)
    _, disp = _planes()
    names = ("ee", "energy", "sums", "centers", "I")

    def f(rows):
        d = {}
        _put(d, "centroid/", names, abi.psf_ee(rows, o, e1, e2, disp, xs, zs, RADII, want_intensity=True)[:5])  # (centers_out: the centroids as used)
        _put(d, "given/", names, abi.psf_ee(rows, o, e1, e2, disp, xs, zs, RADII, centers=np.zeros((M_PLANES, 2)), shape="square")[:5])
        return d

    return _per_rows(f)


# ------------------------------------------------------------------------------------------------ spot read-outs
SPOT_WINDOW = (-1.5 * mm, 2 * mm, -1 * mm, 1 * mm)
SPOT_SHAPES = ((16, 16), (129, 128))  # (the LDS path: 256 bins; the global path: 16 512 > spot_ref.LDS_BINS bins)


def spot_rows(H):
    """H seeded rows [H, 2] over 1.5 x SPOT_WINDOW with the crafted edge rows of spot_ref.window_rows in front"""
    return sr.window_rows(H, SPOT_WINDOW, seed=1234 + H)


def _per_spot_rows(f):
    out = {}
    for H in ROW_COUNTS:
        for k, v in f(spot_rows(H)).items():
            out["H%d/%s" % (H, k)] = v
    return out


@case("spot_pd", "bmo_spot_image")
def spot_image():
    assert SPOT_SHAPES[0][0] * SPOT_SHAPES[0][1] <= sr.LDS_BINS < SPOT_SHAPES[1][0] * SPOT_SHAPES[1][1]

    def f(rows):
        d = {}
        for nx, nz in SPOT_SHAPES:
            img, outside, _ = abi.spot_image(rows, SPOT_WINDOW, nx, nz)
            d["%dx%d/image" % (nx, nz)], d["%dx%d/outside" % (nx, nz)] = img, np.array([outside], dtype=np.int64)
        return d

    return _per_spot_rows(f)


@case("spot_pd", "bmo_spot_stats")
def spot_stats():
    return _per_spot_rows(lambda rows: {"stats": abi.spot_stats(sr.finite_rows(len(rows), seed=77 + len(rows)))[0]})


@case("spot_pd", "bmo_spot_ee")
def spot_ee():
    def f(rows):
        return {shape: abi.spot_ee(rows, (0.1 * mm, -0.05 * mm), RADII * 50, shape=shape)[0] for shape in ("circle", "square")}

    return _per_spot_rows(f)


class _SpotSweep:
    """A Spotdetector moved sideways through a collimated bundle in three configurations, the middle one without roots: 300 and 257 roots."""

    def __enter__(self):
        sd = bmo.Spotdetector(4 * mm)
        bmo.translate3d(sd, [0, 50 * mm, 0])
        system = bmo.System([sd])
        bundle = scenes.disc_bundle(557, center=[0, -10 * mm, 0], direction=[0, 1, 0], diameter=3 * mm, lam=1e-6, jitter=1e-3)

        def configure(c):
            bmo.translate_to3d(sd, [0.2 * mm * c, 50 * mm, -0.1 * mm * c])

        snaps = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)[0]
        self.slot = 0
        _, self.handle, self.lib = bmo.sweep_trace(snaps, bundle, _root_config(300, 257), 100, 0, False, view=False)  # (a detector-only solve)
        return self

    def __exit__(self, *exc):
        self.lib.bmo_result_free(self.handle)


@case("spot_pd", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_spot_image_sweep", "bmo_spot_stats_sweep", "bmo_spot_ee_sweep")
def spot_sweeps():
    out = {}
    windows = np.array([SPOT_WINDOW, (-2 * mm, 2 * mm, -2 * mm, 2 * mm), (-1 * mm, 0.5 * mm, -0.3 * mm, 1.2 * mm)])
    with _SpotSweep() as sw:
        for nx, nz in SPOT_SHAPES:
            _put(out, "%dx%d/" % (nx, nz), ("image", "outside"), abi.spot_image_sweep(sw.handle, sw.slot, 3, windows, nx, nz)[:2])
        out["stats"] = abi.spot_stats_sweep(sw.handle, sw.slot, 3)[0]
        centers = np.array([(0.0, 0.0), (1e-4, 0.0), (-2e-4, 1e-4)])
        for shape in ("circle", "square"):
            _put(out, shape + "/", ("inside", "n_rows"), abi.spot_ee_sweep(sw.handle, sw.slot, 3, centers, RADII * 50, shape=shape)[:2])
    return out


# ------------------------------------------------------------------------------------------------ Photodetector
PD_XS, PD_YS = np.linspace(-1 * mm, 1 * mm, 9), np.linspace(-0.5 * mm, 0.7 * mm, 5)


@case("spot_pd", "bmo_scene_create", "bmo_trace", "bmo_result_view", "bmo_photodetector_field", "bmo_gauss_parameters", "bmo_result_set_gauss_prefix")
def photodetector_field():
    """Three beamlets on a 9 x 5 grid.  field_inout is read and written (include/bmo.h:428): the case hands it zeros, then the first
    call's field again (the sum doubles).  With a prefix of no earlier segments (include/bmo.h:447, "0 for a beamlet without any") the field
    is read once more."""
    system, pd, bundle = pd_scene(3)
    scene = bmo.CompiledScene(system, bundle.lambdas)
    slot = next(i for i, d in enumerate(scene.detectors) if d is pd)
    res, sol = _engine_solve(scene, bundle, R_MAX, None)
    try:
        f = np.zeros((len(PD_XS), len(PD_YS)), dtype=np.complex128)
        sol.photodetector_field(slot, pd.position(), pd.orientation(), PD_XS, PD_YS, f)
        once = f.copy()
        sol.photodetector_field(slot, pd.position(), pd.orientation(), PD_XS, PD_YS, f)
        node = int(res.detector_nodes(slot)[0])
        gp = sol.gauss_parameters(node, np.linspace(0.0, 40 * mm, 7))
        sol.set_gauss_prefix(np.zeros(bundle.n + 1, dtype=np.int32), np.zeros((24, 0)), np.zeros(bundle.n))
        g = np.zeros_like(once)
        sol.photodetector_field(slot, pd.position(), pd.orientation(), PD_XS, PD_YS, g)
    finally:
        sol.free()
    return {"once": once, "twice": f, "gauss_parameters": gp, "with_empty_prefix": g, "det_count": res.det_count}


@case("spot_pd", "bmo_scene_create_sweep", "bmo_trace_sweep", "bmo_photodetector_field_sweep")
def photodetector_field_sweep():
    """K = 3 with an empty configuration and a pose each, three beamlets per configuration with roots.  field_inout is read and written
    (include/bmo.h:478): the case hands it zeros."""
    system, pd, bundle = pd_scene(3)
    p0 = np.array(pd.position(), dtype=np.float64)

    def configure(c):
        bmo.translate_to3d(pd, list(p0 + np.array([0.02 * mm * c, -0.015 * mm * c, 0.1 * mm * c])))
        bmo.xrotate3d(pd, math.radians(0.7 * (1 + c)))

    snaps, poses, _ = bmo.sweep_snapshots(system, bundle.lambdas, 3, configure)
    slot = next(i for i, d in enumerate(snaps[0].detectors) if d is pd)
    tiled = bmo.RayBundle(bundle.kind, np.tile(bundle.planes, (1, 2)))
    _, h, lib = bmo.sweep_trace(snaps, tiled, _root_config(3, 3), R_MAX, 0, True, view=False)
    try:
        dp = C.POINTER(C.c_double)
        pos = np.ascontiguousarray([poses[c][slot][0] for c in range(3)], dtype=np.float64)
        ori = np.ascontiguousarray([np.asarray(poses[c][slot][1]).reshape(9) for c in range(3)], dtype=np.float64)
        nx, ny = len(PD_XS), len(PD_YS)
        buf = np.zeros(2 * 3 * nx * ny)
        abi.check(lib, lib.bmo_photodetector_field_sweep(h, slot, 3, pos.ctypes.data_as(dp), ori.ctypes.data_as(dp), PD_XS.ctypes.data_as(dp),
                                                         PD_YS.ctypes.data_as(dp), nx, ny, buf.ctypes.data_as(dp), None), "bmo_photodetector_field_sweep")
    finally:
        lib.bmo_result_free(h)
    return {"field": buf}


@case("spot_pd", "bmo_selftest")
def selftest():
    lib = abi.load_engine()
    return {"rc": np.array([lib.bmo_selftest(0)], dtype=np.int32)}


# ------------------------------------------------------------------------------------------------ polychromatic
def _poly_rows():
    rows = pr.recolour(_psf_setup()[0][:600])
    rows[[5, 256, 599], 8] = np.nan  # rows of no band
    return rows


@case("poly", "bmo_psf_bands_create", "bmo_psf_bands_info", "bmo_psf_bands_get", "bmo_psf_stats", "bmo_psf_poly_through_focus", "bmo_psf_poly_otf")
def psf_bands_and_poly():
    """The discovery form and the listed form (with a listed band that no row has, second in the list, and NaN keys among the rows); the
    stack with the per-band output; the transform with the combined image."""
    _, o, e1, e2, _ = _psf_setup()
    xs, zs = _axes(5)
    _, disp = _planes()
    rows = _poly_rows()
    k = [pr.wave_number(l) for l in pr.WAVELENGTHS]
    out = {}
    for label, ks in (("discover/", None), ("listed/", [k[2], pr.wave_number(600e-9), k[0]])):
        with abi.psf_bands(rows, ks=ks) as bands:
            out[label + "ks"], out[label + "counts"] = bands.ks, bands.counts
            out[label + "n_rows_unmatched"] = np.array([bands.n_rows, bands.unmatched], dtype=np.int64)
            for b in range(len(bands)):  # the band's rows as a read-out sees them
                ptr, cnt = bands.rows(b)
                out[label + "band%d_stats" % b] = abi.psf_stats(None, o, e1, e2, device=bands.device, hits_device_ptr=ptr, n_hits=cnt)[0]
            coeffs = np.array([0.5, 0.3, 0.2])[:len(bands)]
            _put(out, label + "stack/", ("I", "I_b"), abi.psf_poly_through_focus(bands, o, e1, e2, disp, xs, zs, coeffs, want_bands=True)[:2])
            _put(out, label + "stack_plain/", ("I", "I_b"), abi.psf_poly_through_focus(bands, o, e1, e2, disp, xs, zs, coeffs)[:2])
            _put(out, label + "otf/", ("mtf", "otf", "sums", "I"), abi.psf_poly_otf(bands, o, e1, e2, disp, xs, zs, coeffs, FREQS, want_intensity=True)[:4])
    with abi.psf_bands(rows[:0]) as bands:  # no rows: no band
        out["empty/n"] = np.array([len(bands), bands.n_rows, bands.unmatched], dtype=np.int64)
        _put(out, "empty/stack/", ("I", "I_b"), abi.psf_poly_through_focus(bands, o, e1, e2, disp, xs, zs, np.zeros(0), want_bands=True)[:2])
        _put(out, "empty/otf/", ("mtf", "otf", "sums", "I"), abi.psf_poly_otf(bands, o, e1, e2, disp, xs, zs, np.zeros(0), FREQS, want_intensity=True)[:4])
    return out


# ------------------------------------------------------------------------------------------------ running
def run(f):
    """The case's dict, every value as a contiguous array."""
    return {k: np.ascontiguousarray(v) for k, v in f().items()}


def bits(a):
    """An array as the integers that hold it: int32 stays, everything else of 8-byte elements (complex as pairs of doubles) as uint64."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.int32:
        return a
    if a.dtype == np.bool_:
        return a.view(np.uint8)
    if np.iscomplexobj(a):
        a = a.astype(np.complex128, copy=False).view(np.float64)
    assert a.dtype.itemsize == 8, a.dtype
    return a.view(np.uint64)


def differences(got, want):
    """Keys whose arrays differ in shape, type or any bit, with the first differing index."""
    bad = []
    for k in sorted(set(got) | set(want)):
        if k not in got or k not in want:
            bad.append((k, "missing"))
            continue
        g, w = bits(got[k]), bits(want[k])
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append((k, "shape/dtype", g.shape, w.shape))
        elif not np.array_equal(g, w):
            idx = np.argwhere(g != w)
            bad.append((k, "%d of %d words" % (len(idx), g.size), idx[0].tolist()))
    return bad
