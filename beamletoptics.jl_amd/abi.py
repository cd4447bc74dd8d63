"""ctypes mirror of include/bmo.h and the loader of the HIP engine (libbmo_hip.so).

There is NO CPU fallback: `load_engine()` raises if the compiled HIP library is missing, and
every trace entry point of the library itself fails without a GPU (BMO_ERR_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

ABI_VERSION = 1
NPARAM = 8

VIEW_HITS, VIEW_LAST_SEGMENT, VIEW_SEGMENTS = 1, 2, 4  # bmo_result_view_select masks

PLANES_IN = {0: 8, 1: 14, 2: 25}
PLANES_REC = {0: 11, 1: 17, 2: 33}

# BMO_SPOT_STAT_*: columns of the spot statistics (bmo_spot_stats)
SPOT_STAT_N = 12
(SPOT_N, SPOT_CX, SPOT_CZ, SPOT_X_MIN, SPOT_X_MAX, SPOT_Z_MIN, SPOT_Z_MAX, SPOT_MXX, SPOT_MZZ, SPOT_MXZ, SPOT_RMS_R, SPOT_GEO_R) = range(SPOT_STAT_N)

# BMO_PSF_STAT_*: columns of the wavefront statistics of PSF rows (bmo_psf_stats)
PSF_STAT_N = 21
(PSF_N, PSF_S, PSF_CX, PSF_CZ, PSF_X_MIN, PSF_X_MAX, PSF_Z_MIN, PSF_Z_MAX, PSF_HWX, PSF_HWZ, PSF_X_REF, PSF_Z_REF, PSF_W_MEAN, PSF_W_RMS, PSF_W_LO,
 PSF_W_HI, PSF_F_RE, PSF_F_IM, PSF_STREHL, PSF_K_MIN, PSF_K_MAX) = range(PSF_STAT_N)

# BMO_ZERNIKE_*: columns of the info row of the Zernike read-out (bmo_psf_zernike)
ZERN_INFO_N = 13
ZERN_MAX_ORDER = 6
(ZERN_N, ZERN_STATUS, ZERN_S, ZERN_X_REF, ZERN_Z_REF, ZERN_U0, ZERN_V0, ZERN_RHO, ZERN_W_MEAN, ZERN_FIT_RMS, ZERN_E_LO, ZERN_E_HI,
 ZERN_N_OUT) = range(ZERN_INFO_N)

# BMO_OPD_*: columns of the info row of the OPD map read-out (bmo_psf_opd_map); the first thirteen are the Zernike read-out's
OPD_INFO_N = 20
OPD_MAX_N = 4096
(OPD_N, OPD_STATUS, OPD_S, OPD_X_REF, OPD_Z_REF, OPD_U0, OPD_V0, OPD_RHO, OPD_W_MEAN, OPD_E_RMS, OPD_E_LO, OPD_E_HI, OPD_N_OUT, OPD_N_OUTSIDE, OPD_N_BAD,
 OPD_N_FILLED, OPD_SH_Q, OPD_SH_P, OPD_MAP_LO, OPD_MAP_HI) = range(OPD_INFO_N)

# BMO_FOCUS_STAT_*: columns of the focus statistics (bmo_psf_focus_stats)
FOCUS_STAT_N = 12
(FOCUS_N, FOCUS_S, FOCUS_CX, FOCUS_CZ, FOCUS_X_MIN, FOCUS_X_MAX, FOCUS_Z_MIN, FOCUS_Z_MAX, FOCUS_HWX, FOCUS_HWZ, FOCUS_RMS_R, FOCUS_MAX_R) = range(FOCUS_STAT_N)

PSF_MAX_BANDS = 64  # BMO_PSF_MAX_BANDS: the wavelength bands of one bmo_psf_bands handle

NODE_MISS, NODE_STOPPED, NODE_RMAX, NODE_SPLIT, NODE_DETECTED, NODE_ERR_UNIT, NODE_GAUSS_DIVERGED, NODE_BLOCKED, NODE_ERR_ORTHO = (
    1, 2, 4, 8, 16, 32, 64, 128, 256)


class Shape(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("child_begin", C.c_int32), ("child_count", C.c_int32), ("tri_begin", C.c_int32),
        ("tri_count", C.c_int32), ("flags", C.c_int32),
        ("pos", C.c_double * 3), ("dir", C.c_double * 9), ("tdir", C.c_double * 9), ("p", C.c_double * NPARAM),
        ("bs_center", C.c_double * 3), ("bs_radius", C.c_double),
    ]


class Object(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("shape", C.c_int32 * 3), ("medium", C.c_int32 * 2), ("detector", C.c_int32), ("reserved", C.c_int32),
        ("reflectance", C.c_double), ("transmittance", C.c_double), ("cutoff", C.c_double), ("jones", C.c_double * 18),
    ]


class SceneDesc(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_objects", C.c_int32), ("n_shapes", C.c_int32), ("n_children", C.c_int32),
        ("n_tris", C.c_int32), ("n_media", C.c_int32), ("n_lambda", C.c_int32), ("n_detectors", C.c_int32),
        ("objects", C.POINTER(Object)), ("shapes", C.POINTER(Shape)), ("children", C.POINTER(C.c_int32)),
        ("tris", C.POINTER(C.c_double)), ("n_table", C.POINTER(C.c_double)), ("lambdas", C.POINTER(C.c_double)),
        ("coefs", C.POINTER(C.c_double)),
        ("eps_srf", C.c_double), ("eps_ray", C.c_double), ("eps_ins", C.c_double), ("mt_keps", C.c_double),
        ("mt_leps", C.c_double), ("grad_h", C.c_double), ("march_iters", C.c_int32), ("n_coefs", C.c_int32),
    ]


class RayBatch(C.Structure):
    _fields_ = [("n", C.c_int64), ("kind", C.c_int32), ("n_planes", C.c_int32), ("planes", C.POINTER(C.c_double)),
                ("lambda_idx", C.POINTER(C.c_int32))]


class TraceOpts(C.Structure):
    _fields_ = [("r_max", C.c_int32), ("device", C.c_int32), ("record_segments", C.c_int32), ("max_beams", C.c_int32)]


class ResultView(C.Structure):
    _fields_ = [
        ("n_roots", C.c_int64), ("n_nodes", C.c_int64), ("n_records", C.c_int64), ("n_intersect_calls", C.c_int64),
        ("n_steps", C.c_int32), ("beam_kind", C.c_int32), ("rec_planes", C.c_int32), ("n_detectors", C.c_int32),
        ("node_root", C.POINTER(C.c_int32)), ("node_parent", C.POINTER(C.c_int32)), ("node_first_child", C.POINTER(C.c_int32)),
        ("node_first_rec", C.POINTER(C.c_int32)), ("node_nseg", C.POINTER(C.c_int32)), ("node_status", C.POINTER(C.c_int32)),
        ("node_aux", C.POINTER(C.c_double)),
        ("rec_obj", C.POINTER(C.c_int32)), ("rec_shape", C.POINTER(C.c_int32)), ("rec", C.POINTER(C.c_double)),
        ("det_count", C.POINTER(C.c_int64)), ("det_offset", C.POINTER(C.c_int64)), ("det_node", C.POINTER(C.c_int32)),
        ("det_data", C.POINTER(C.c_double)),
    ]


def _out(shape, dtype=float):
    """Every buffer a C entry writes is allocated here, and nowhere else in this module.  Zeros in production; tests/test_state_independence_gpu.py
    swaps this for a filler of 0x7FF8DEAD words, as a caller that hands the entries uninitialised memory (julia/GPUSystem.jl) would."""
    return np.zeros(shape, dtype=dtype)


def _np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class TraceResult:
    """Host copy of a bmo_trace_result_view (arrays are numpy copies; see include/bmo.h for the layout)."""

    def __init__(self, v):
        nn, nr = int(v.n_nodes), int(v.n_records)
        self.n_roots = int(v.n_roots)
        self.n_nodes = nn
        self.n_records = nr
        self.n_intersect_calls = int(v.n_intersect_calls)
        self.n_steps = int(v.n_steps)
        self.beam_kind = int(v.beam_kind)
        self.rec_planes = int(v.rec_planes)
        self.n_detectors = int(v.n_detectors)
        self.node_root = _np(v.node_root, nn, np.int32)
        self.node_parent = _np(v.node_parent, nn, np.int32)
        self.node_first_child = _np(v.node_first_child, nn, np.int32)
        self.node_first_rec = _np(v.node_first_rec, nn, np.int32)
        self.node_nseg = _np(v.node_nseg, nn, np.int32)
        self.node_status = _np(v.node_status, nn, np.int32)
        self.node_aux = _np(v.node_aux, nn * 4, np.float64).reshape(nn, 4)
        self.rec_obj = _np(v.rec_obj, nr, np.int32)
        self.rec_shape = _np(v.rec_shape, nr, np.int32)
        self.rec = _np(v.rec, nr * self.rec_planes, np.float64).reshape(self.rec_planes, nr)
        nd = self.n_detectors
        self.det_count = _np(v.det_count, nd, np.int64)
        self.det_offset = _np(v.det_offset, nd, np.int64)
        tot = int(self.det_count.sum())
        if not v.det_data:  # a selective view without BMO_VIEW_HITS: counts only
            tot = 0
        self.det_node = _np(v.det_node, tot, np.int32)
        self.det_data = _np(v.det_data, tot * 9, np.float64).reshape(tot, 9)

    def as_view(self):
        """A ResultView over this object's numpy arrays (valid while `self` is alive) — e.g. the `prev` of a test emulator."""
        v = ResultView()
        v.n_roots, v.n_nodes, v.n_records, v.n_intersect_calls = self.n_roots, self.n_nodes, self.n_records, self.n_intersect_calls
        v.n_steps, v.beam_kind, v.rec_planes, v.n_detectors = self.n_steps, self.beam_kind, self.rec_planes, self.n_detectors
        keep = []
        for name, ct in (("node_root", C.c_int32), ("node_parent", C.c_int32), ("node_first_child", C.c_int32), ("node_first_rec", C.c_int32),
                         ("node_nseg", C.c_int32), ("node_status", C.c_int32), ("node_aux", C.c_double), ("rec_obj", C.c_int32),
                         ("rec_shape", C.c_int32), ("rec", C.c_double), ("det_count", C.c_int64), ("det_offset", C.c_int64),
                         ("det_node", C.c_int32), ("det_data", C.c_double)):
            a = np.ascontiguousarray(getattr(self, name))
            keep.append(a)
            setattr(v, name, a.ctypes.data_as(C.POINTER(ct)))
        self._view_keep = keep
        return v

    def detector_hits(self, slot):
        o, c = int(self.det_offset[slot]), int(self.det_count[slot])
        return self.det_data[o:o + c]

    def detector_nodes(self, slot):
        o, c = int(self.det_offset[slot]), int(self.det_count[slot])
        return self.det_node[o:o + c]


_HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_PATH = os.environ.get("BMO_ENGINE_LIB") or os.path.join(_HERE, "csrc", "libbmo_hip.so")  # env: A/B builds of the HIP engine
_engine = None


class EngineMissing(RuntimeError):
    pass


def _check_source_hash(lib):
    """Refuse a library that was not built from the sources next to it (a stale, git-ignored .so pushed along with newer sources), or
    with other compiler flags (bit parity needs -ffp-contract=off & co.).  The build script next to the package says what is wanted:
    its source list and flag list decide.  Skipped for an explicitly chosen build (BMO_ENGINE_LIB: A/B runs) and where there is no
    build script or the sources are not there to compare with (an installed copy of the package)."""
    if os.environ.get("BMO_ENGINE_LIB"):
        return
    build = _build_script(os.path.dirname(_HERE))
    if build is None or not all(os.path.exists(p) for p in build.engine_sources()):
        return

    def built(symbol):
        try:
            f = getattr(lib, symbol)
            f.restype = C.c_char_p
            return f().decode()
        except AttributeError:
            return None

    rebuild = "rebuild it with `python -c 'import __graft_entry__ as g; g.build()'`"
    got, want = built("bmo_source_hash"), build.source_hash()
    if got != want:
        raise EngineMissing(f"{ENGINE_PATH} was not built from the sources in this tree (source hash {got!r} != {want[:16]}...): {rebuild}")
    got, want = built("bmo_build_flags_hash"), build.flags_hash()
    if got != want:
        raise EngineMissing(f"{ENGINE_PATH} was built with other compiler flags than __graft_entry__.HIP_FLAGS (flags hash {got!r} != {want!r}): {rebuild}")


def _build_script(root):
    """The build script next to the package as a module (None where there is none, or where it does not load)."""
    path = os.path.join(root, "__graft_entry__.py")
    if not os.path.exists(path):
        return None
    import importlib.util

    spec = importlib.util.spec_from_file_location("_bmo_graft_entry", path)
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
        return mod
    except Exception:
        return None


def load_engine():
    """Load the HIP engine.  Fails loudly when the compiled library is missing or stale."""
    global _engine
    if _engine is not None:
        return _engine
    if not os.path.exists(ENGINE_PATH):
        raise EngineMissing(
            f"{ENGINE_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(ENGINE_PATH)
    _check_source_hash(lib)
    vp = C.c_void_p
    lib.bmo_version.restype = C.c_int
    lib.bmo_last_error.restype = C.c_char_p
    lib.bmo_device_count.restype = C.c_int
    lib.bmo_selftest.argtypes = [C.c_int32]
    lib.bmo_selftest.restype = C.c_int
    lib.bmo_jl_trig.argtypes = [C.c_int32, C.c_double, C.c_double]
    lib.bmo_jl_trig.restype = C.c_double
    lib.bmo_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(vp)]
    lib.bmo_scene_mesh_bvh.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.bmo_mesh_nearest_host.argtypes = [vp, C.c_int32, C.c_int64] + [C.POINTER(C.c_double)] * 3 + [C.POINTER(C.c_int32)]
    lib.bmo_scene_destroy.argtypes = [vp]
    lib.bmo_pool_release.argtypes = []
    lib.bmo_pool_release.restype = C.c_int
    lib.bmo_trace.argtypes = [vp, C.POINTER(RayBatch), C.POINTER(TraceOpts), C.POINTER(vp)]
    lib.bmo_batch_upload.argtypes = [vp, C.POINTER(RayBatch), C.c_int32, C.POINTER(vp)]
    lib.bmo_batch_free.argtypes = [vp]
    lib.bmo_trace_device.argtypes = [vp, vp, C.POINTER(TraceOpts), C.POINTER(vp)]
    lib.bmo_result_device_hits.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int64)]
    lib.bmo_result_copy_hits.argtypes = [vp, C.c_int32, C.c_void_p, C.c_int64]
    lib.bmo_result_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.bmo_result_counts.argtypes = [vp] + [C.POINTER(C.c_int64)] * 4
    lib.bmo_result_view.argtypes = [vp, C.POINTER(ResultView)]
    lib.bmo_result_view_select.argtypes = [vp, C.c_uint32, C.POINTER(ResultView)]
    lib.bmo_result_copy_hit_columns.argtypes = [vp, C.c_int32, C.c_int32, C.c_void_p, C.c_int64]
    lib.bmo_result_free.argtypes = [vp]
    lib.bmo_retrace.argtypes = [vp, C.POINTER(RayBatch), vp, C.POINTER(TraceOpts), C.POINTER(vp)]
    lib.bmo_retrace_device.argtypes = [vp, vp, vp, C.POINTER(TraceOpts), C.POINTER(vp)]
    dp = C.POINTER(C.c_double)
    lib.bmo_photodetector_field.argtypes = [vp, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp]
    lib.bmo_gauss_parameters.argtypes = [vp, C.c_int64, dp, C.c_int32, dp]
    lib.bmo_result_set_gauss_prefix.argtypes = [vp, C.c_int64, C.POINTER(C.c_int32), dp, dp]
    lib.bmo_psf_intensity.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp, dp]
    lib.bmo_scene_create_sweep.argtypes = [C.POINTER(SceneDesc), C.c_int32, C.POINTER(vp)]
    lib.bmo_trace_sweep.argtypes = [vp, C.POINTER(RayBatch), C.POINTER(C.c_int32), C.POINTER(TraceOpts), C.POINTER(vp)]
    lib.bmo_photodetector_field_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp]
    lib.bmo_psf_intensity_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, dp, dp]
    ip = C.POINTER(C.c_int64)
    lib.bmo_spot_image.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, dp, C.c_int32, C.c_int32, C.c_int32, ip, ip, dp]
    lib.bmo_spot_image_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32, C.c_int32, ip, ip, dp]
    lib.bmo_spot_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, dp, dp]
    lib.bmo_spot_stats_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp]
    lib.bmo_psf_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp]
    lib.bmo_psf_stats_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, dp]
    lib.bmo_psf_zernike.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp, dp, dp]
    lib.bmo_psf_zernike_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, dp, dp, dp]
    lib.bmo_psf_opd_map.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, ip, ip, dp, dp]
    lib.bmo_psf_opd_map_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, C.c_int32, dp, dp, ip, ip, dp, dp]
    lib.bmo_psf_through_focus.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, C.c_int32, dp, dp, dp]
    lib.bmo_psf_focus_stats.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, dp]
    lib.bmo_result_psf_rows.argtypes = [vp, C.c_int32, C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.bmo_psf_geo_otf.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, dp, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, dp, dp]
    lib.bmo_psf_otf.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp]
    # include/bmo_sweep_readout.h
    lib.bmo_psf_focus_stats_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, dp]
    lib.bmo_psf_through_focus_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, dp, dp]
    lib.bmo_psf_geo_otf_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, dp, C.c_int32, dp, C.c_int32, dp, dp, dp, dp]
    lib.bmo_psf_otf_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, C.c_int32, dp, dp, dp, dp, dp]
    lib.bmo_spot_ee.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, dp, C.c_int32, dp, C.c_int32, C.c_int32, ip, dp]
    lib.bmo_spot_ee_sweep.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32, dp, C.c_int32, ip, ip, dp]
    lib.bmo_psf_geo_ee.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, ip, dp, dp]
    lib.bmo_psf_ee.argtypes = [C.c_void_p, C.c_int64, C.c_int32, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, dp]
    lib.bmo_psf_bands_create.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, dp, C.c_int32, C.POINTER(vp), dp]
    lib.bmo_psf_bands_info.argtypes = [vp, C.POINTER(C.c_int32), ip, ip, C.POINTER(C.c_int32)]
    lib.bmo_psf_bands_get.argtypes = [vp, C.c_int32, dp, C.POINTER(C.POINTER(C.c_double)), ip]
    lib.bmo_psf_bands_free.argtypes = [vp]
    lib.bmo_psf_poly_through_focus.argtypes = [vp, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, dp, dp, dp]
    lib.bmo_psf_poly_otf.argtypes = [vp, dp, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, dp, C.c_int32, dp, dp, dp, dp, dp]
    _engine = lib
    return lib


def check(lib, rc, what):
    if rc != 0:
        msg = lib.bmo_last_error()
        raise RuntimeError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def pool_release():
    """bmo_pool_release: gives every block the device pool keeps back to the driver (the next allocations are fresh ones)."""
    lib = load_engine()
    check(lib, lib.bmo_pool_release(), "bmo_pool_release")


def _psf_rows(hits, hits_device_ptr, n_hits):
    """(pointer, row count, on_device, keep-alive) of the PSF rows of a single read-out."""
    if hits_device_ptr is not None:
        return C.c_void_p(int(hits_device_ptr)), int(n_hits), 1, None
    h = np.ascontiguousarray(np.asarray(hits, dtype=np.float64).reshape(-1, 9))
    return h.ctypes.data_as(C.c_void_p), len(h), 0, h


def _per_config(v, K1, cols):
    """An optional per-configuration argument of a _sweep form as [K1, cols]: None stays None, one row counts for all."""
    if v is None:
        return None
    v = np.asarray(v, dtype=np.float64)
    return np.ascontiguousarray(np.tile(v, (K1, 1)) if v.ndim == 1 else v.reshape(K1, cols))


def psf_intensity(hits, origin, e1, e2, xs, zs, device=0, hits_device_ptr=None, n_hits=None, want_field=False):
    """bmo_psf_intensity: returns (I[n, n] indexed [i, j], field or None, kernel_ms).  `hits` is a host [H, 9] array, or pass
    `hits_device_ptr` + `n_hits` for a buffer already resident on `device` (bmo_result_device_hits)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)

    def arr(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, a.ctypes.data_as(dp)

    (o, op), (a1, e1p), (a2, e2p), (x, xp), (z, zp) = arr(origin), arr(e1), arr(e2), arr(xs), arr(zs)
    n = len(x)
    if len(z) != n:
        raise ValueError("xs and zs must have the same length")
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    out = _out(n * n)
    fld = _out(2 * n * n) if want_field else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_intensity(hp, nh, on_dev, op, e1p, e2p, xp, zp, n, int(device), out.ctypes.data_as(dp),
                                     fld.ctypes.data_as(dp) if want_field else None, C.byref(ms)), "bmo_psf_intensity")
    field = (fld[0::2] + 1j * fld[1::2]).reshape(n, n).T.copy() if want_field else None
    return out.reshape(n, n).T.copy(), field, ms.value


def psf_intensity_sweep(res_handle, detector, n_configs, origins, e1s, e2s, xs, zs, want_field=False):
    """bmo_psf_intensity_sweep on the result handle `res_handle`: origins / e1s / e2s [K, 3], xs / zs [K, n].  Returns (I[K, n, n] indexed
    [c, i, j], field [K, n, n] or None, kernel_ms); configuration c equals psf_intensity on its rows at its axes and pose, bit for bit."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)

    def arr(a, cols):
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(K, cols))
        return a, a.ctypes.data_as(dp)

    xs = np.asarray(xs, dtype=np.float64)
    n = xs.shape[-1]
    (o, op), (a1, e1p), (a2, e2p), (x, xp), (z, zp) = arr(origins, 3), arr(e1s, 3), arr(e2s, 3), arr(xs, n), arr(zs, n)
    out = _out(K * n * n)
    fld = _out(2 * K * n * n) if want_field else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_intensity_sweep(res_handle, int(detector), K, op, e1p, e2p, xp, zp, n, out.ctypes.data_as(dp),
                                           fld.ctypes.data_as(dp) if want_field else None, C.byref(ms)), "bmo_psf_intensity_sweep")
    field = np.ascontiguousarray((fld[0::2] + 1j * fld[1::2]).reshape(K, n, n).transpose(0, 2, 1)) if want_field else None
    return np.ascontiguousarray(out.reshape(K, n, n).transpose(0, 2, 1)), field, ms.value


def _spot_rows(rows, rows_device_ptr, n_rows, row_cols):
    """(pointer, row count, columns, on_device, keep-alive) of the rows of a single spot read-out."""
    if rows_device_ptr is not None:
        return C.c_void_p(int(rows_device_ptr)), int(n_rows), int(row_cols), 1, None
    r = np.asarray(rows, dtype=np.float64)
    r = np.ascontiguousarray(r if r.ndim == 2 else r.reshape(-1, 2))
    return r.ctypes.data_as(C.c_void_p), r.shape[0], r.shape[1], 0, r


def spot_image(rows, window, nx, nz=None, device=0, rows_device_ptr=None, n_rows=None, row_cols=9):
    """bmo_spot_image: the rows [n, 2..9] (x in column 0, z in column 1) binned on window (x0, x1, z0, z1) by the floor rule of include/bmo.h.
    Returns (counts int64 [nx, nz] indexed [i, j], outside, kernel_ms).  `rows` is a host array, or pass `rows_device_ptr` + `n_rows` +
    `row_cols` for rows already resident on `device` (bmo_result_device_hits: 9 columns)."""
    lib = load_engine()
    nz = nx if nz is None else nz
    rp, n, cols, on_dev, keep = _spot_rows(rows, rows_device_ptr, n_rows, row_cols)
    w = np.ascontiguousarray(window, dtype=np.float64).reshape(4)
    img = _out(max(int(nx) * int(nz), 0), dtype=np.int64)
    out = C.c_int64()
    ms = C.c_double()
    check(lib, lib.bmo_spot_image(rp, n, cols, on_dev, w.ctypes.data_as(C.POINTER(C.c_double)), int(nx), int(nz), int(device),
                                  img.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(out), C.byref(ms)), "bmo_spot_image")
    return img.reshape(nz, nx).T.copy(), out.value, ms.value


def spot_image_sweep(res_handle, detector, n_configs, windows, nx, nz=None):
    """bmo_spot_image_sweep on the result handle `res_handle`: windows [K, 4] (or one window for all).  Returns (counts int64 [K, nx, nz]
    indexed [c, i, j], outside int64 [K], kernel_ms); configuration c equals spot_image on its rows."""
    lib = load_engine()
    K = int(n_configs)
    nz = nx if nz is None else nz
    w = _per_config(windows, max(K, 1), 4)
    img = _out(max(K, 1) * max(int(nx) * int(nz), 0), dtype=np.int64)
    out = _out(max(K, 1), dtype=np.int64)
    ms = C.c_double()
    ip = C.POINTER(C.c_int64)
    check(lib, lib.bmo_spot_image_sweep(res_handle, int(detector), K, w.ctypes.data_as(C.POINTER(C.c_double)), int(nx), int(nz), img.ctypes.data_as(ip),
                                        out.ctypes.data_as(ip), C.byref(ms)), "bmo_spot_image_sweep")
    return np.ascontiguousarray(img.reshape(K, nz, nx).transpose(0, 2, 1)), out, ms.value


def spot_stats(rows, device=0, rows_device_ptr=None, n_rows=None, row_cols=9):
    """bmo_spot_stats: the twelve statistics (SPOT_* columns) of the rows, two passes on the device.  Returns (stats [12], kernel_ms)."""
    lib = load_engine()
    rp, n, cols, on_dev, keep = _spot_rows(rows, rows_device_ptr, n_rows, row_cols)
    st = _out(SPOT_STAT_N)
    ms = C.c_double()
    check(lib, lib.bmo_spot_stats(rp, n, cols, on_dev, int(device), st.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ms)), "bmo_spot_stats")
    return st, ms.value


def spot_stats_sweep(res_handle, detector, n_configs):
    """bmo_spot_stats_sweep on the result handle `res_handle`.  Returns (stats [K, 12], kernel_ms); row c equals spot_stats on the rows of
    configuration c bit for bit."""
    lib = load_engine()
    K = int(n_configs)
    st = _out((max(K, 1), SPOT_STAT_N))
    ms = C.c_double()
    check(lib, lib.bmo_spot_stats_sweep(res_handle, int(detector), K, st.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ms)), "bmo_spot_stats_sweep")
    return st[:K], ms.value


def psf_stats(hits, origin, e1, e2, ref=None, device=0, hits_device_ptr=None, n_hits=None):
    """bmo_psf_stats: the 21 wavefront statistics (PSF_* columns) of PSF rows at the detector pose (origin, e1, e2), three passes on the
    device.  ref: the reference point (x, z) in detector-local coordinates, None for the centroid.  `hits` is a host [H, 9] array, or pass
    `hits_device_ptr` + `n_hits` for rows already resident on `device` (bmo_result_device_hits).  Returns (stats [21], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    r = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64).reshape(2)
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    st = _out(PSF_STAT_N)
    ms = C.c_double()
    check(lib, lib.bmo_psf_stats(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), None if r is None else r.ctypes.data_as(dp),
                                 int(device), st.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_stats")
    return st, ms.value


def psf_stats_sweep(res_handle, detector, n_configs, origins, e1s, e2s, ref=None):
    """bmo_psf_stats_sweep on the result handle `res_handle`: origins / e1s / e2s [K, 3], ref None (every configuration's centroid), one
    (x, z) for all or [K, 2].  Returns (stats [K, 21], kernel_ms); row c equals psf_stats on the rows of configuration c bit for bit."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    K1 = max(K, 1)
    o, a1, a2 = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(K1, 3)) for v in (origins, e1s, e2s))
    r = _per_config(ref, K1, 2)
    st = _out((K1, PSF_STAT_N))
    ms = C.c_double()
    check(lib, lib.bmo_psf_stats_sweep(res_handle, int(detector), K, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp),
                                       None if r is None else r.ctypes.data_as(dp), st.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_stats_sweep")
    return st[:K], ms.value


def psf_through_focus(hits, origin, e1, e2, displacements, xs, zs, device=0, hits_device_ptr=None, n_hits=None, want_field=False):
    """bmo_psf_through_focus: the PSF of the rows on the grid (xs, zs) displaced by each of `displacements` [M, 3] (world vectors), in one
    pass over the rows.  Returns (I[M, n, n] indexed [m, i, j], field [M, n, n] or None, kernel_ms); the plane with a zero displacement
    equals psf_intensity bit for bit.  `hits` is a host [H, 9] array, or pass `hits_device_ptr` + `n_hits` for resident rows."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    d = np.ascontiguousarray(np.asarray(displacements, dtype=np.float64).reshape(-1, 3))
    x, z = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(zs, dtype=np.float64)
    n, M = len(x), len(d)
    if len(z) != n:
        raise ValueError("xs and zs must have the same length")
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    out = _out(M * n * n)
    fld = _out(2 * M * n * n) if want_field else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_through_focus(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), d.ctypes.data_as(dp), M,
                                         x.ctypes.data_as(dp), z.ctypes.data_as(dp), n, int(device), out.ctypes.data_as(dp),
                                         fld.ctypes.data_as(dp) if want_field else None, C.byref(ms)), "bmo_psf_through_focus")
    field = np.ascontiguousarray((fld[0::2] + 1j * fld[1::2]).reshape(M, n, n).transpose(0, 2, 1)) if want_field else None
    return np.ascontiguousarray(out.reshape(M, n, n).transpose(0, 2, 1)), field, ms.value


def psf_focus_stats(hits, origin, e1, e2, axis, offsets, device=0, hits_device_ptr=None, n_hits=None):
    """bmo_psf_focus_stats: the twelve spot statistics (FOCUS_* columns) of the rows propagated along their directions to the detector
    plane moved by offsets[m] * axis, two passes on the device.  Returns (stats [M, 12], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2, ax = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2, axis))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64).reshape(-1))
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    st = _out((len(off), FOCUS_STAT_N))
    ms = C.c_double()
    check(lib, lib.bmo_psf_focus_stats(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), ax.ctypes.data_as(dp),
                                       off.ctypes.data_as(dp), len(off), int(device), st.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_focus_stats")
    return st, ms.value


def _freqs(freqs):
    """Frequencies (fx, fz) in cycles per metre as a contiguous [nf, 2] array."""
    return np.ascontiguousarray(np.asarray(freqs, dtype=np.float64).reshape(-1, 2))


def psf_geo_otf(hits, origin, e1, e2, axis, offsets, freqs, centers=None, device=0, hits_device_ptr=None, n_hits=None):
    """bmo_psf_geo_otf: the geometric transfer function T(f) = sum proj cis(-2 pi (fx x + fz z)) of the rows propagated to the detector plane
    moved by offsets[m] * axis, at the frequencies `freqs` [nf, 2] (cycles per metre, local x and z); centers: None or [M, 2], the point of
    each plane the phase is counted from.  Returns (mtf [M, nf], otf [M, nf] complex, sums [M], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2, ax = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2, axis))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64).reshape(-1))
    fq = _freqs(freqs)
    M, nf = len(off), len(fq)
    cen = None if centers is None else np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(M, 2))
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    otf, mtf, sums = _out((M, nf, 2)), _out((M, nf)), _out(M)
    ms = C.c_double()
    check(lib, lib.bmo_psf_geo_otf(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), ax.ctypes.data_as(dp), off.ctypes.data_as(dp),
                                   None if cen is None else cen.ctypes.data_as(dp), M, fq.ctypes.data_as(dp), nf, int(device), otf.ctypes.data_as(dp),
                                   mtf.ctypes.data_as(dp), sums.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_geo_otf")
    return mtf, otf[..., 0] + 1j * otf[..., 1], sums, ms.value


def psf_otf(hits, origin, e1, e2, displacements, xs, zs, freqs, device=0, hits_device_ptr=None, n_hits=None, want_intensity=False):
    """bmo_psf_otf: the transform of the through-focus stack (psf_through_focus of the same arguments, kept on the device) at the frequencies
    `freqs` [nf, 2] (cycles per metre).  Returns (mtf [M, nf], otf [M, nf] complex, sums [M], I[M, n, n] indexed [m, i, j] or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    d = np.ascontiguousarray(np.asarray(displacements, dtype=np.float64).reshape(-1, 3))
    x, z = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(zs, dtype=np.float64)
    fq = _freqs(freqs)
    n, M, nf = len(x), len(d), len(fq)
    if len(z) != n:
        raise ValueError("xs and zs must have the same length")
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    otf, mtf, sums = _out((M, nf, 2)), _out((M, nf)), _out(M)
    img = _out(M * n * n) if want_intensity else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_otf(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), d.ctypes.data_as(dp), M, x.ctypes.data_as(dp),
                               z.ctypes.data_as(dp), n, fq.ctypes.data_as(dp), nf, int(device), otf.ctypes.data_as(dp), mtf.ctypes.data_as(dp),
                               sums.ctypes.data_as(dp), img.ctypes.data_as(dp) if want_intensity else None, C.byref(ms)), "bmo_psf_otf")
    I = np.ascontiguousarray(img.reshape(M, n, n).transpose(0, 2, 1)) if want_intensity else None
    return mtf, otf[..., 0] + 1j * otf[..., 1], sums, I, ms.value


# The through-focus and MTF read-outs of a sweep (include/bmo_sweep_readout.h): `res_handle` a result handle, K = n_configs, poses [K, 3].
# Block c of every output equals the single wrapper above on the rows of configuration c with configuration c's arguments, bit for bit.
def _sweep_args(K, *arrays):
    """[(contiguous FP64 array of shape (K,) + tail, its pointer), ...] for (array, tail) pairs; a pointer of None for an array of None."""
    dp = C.POINTER(C.c_double)
    out = []
    for a, tail in arrays:
        a = None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape((max(K, 1),) + tuple(tail)))
        out.append((a, None if a is None else a.ctypes.data_as(dp)))
    return out


def _sweep_planes(K, v):
    """offsets of a sweep as [K, M]: one list counts for every configuration."""
    v = np.asarray(v, dtype=np.float64)
    return np.ascontiguousarray(np.tile(v.reshape(1, -1), (max(K, 1), 1)) if v.ndim <= 1 else v.reshape(max(K, 1), -1))


def psf_focus_stats_sweep(res_handle, detector, n_configs, origins, e1s, e2s, axes, offsets):
    """bmo_psf_focus_stats_sweep: axes [K, 3], offsets [K, M] (or one list [M] for all).  Returns (stats [K, M, 12], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    off = _sweep_planes(K, offsets)
    M = off.shape[1]
    (o, op), (a1, e1p), (a2, e2p), (ax, axp) = _sweep_args(K, (origins, (3,)), (e1s, (3,)), (e2s, (3,)), (axes, (3,)))
    st = _out((max(K, 1), M, FOCUS_STAT_N))
    ms = C.c_double()
    check(lib, lib.bmo_psf_focus_stats_sweep(res_handle, int(detector), K, op, e1p, e2p, axp, off.ctypes.data_as(dp), M, st.ctypes.data_as(dp), C.byref(ms)),
          "bmo_psf_focus_stats_sweep")
    return st[:K], ms.value


def psf_through_focus_sweep(res_handle, detector, n_configs, origins, e1s, e2s, displacements, xs, zs, want_field=False):
    """bmo_psf_through_focus_sweep: displacements [K, M, 3], xs / zs [K, n].  Returns (I[K, M, n, n] indexed [c, m, i, j], field [K, M, n, n]
    or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    K1 = max(K, 1)
    n = np.asarray(xs).shape[-1]
    M = np.asarray(displacements).size // (3 * K1)
    (o, op), (a1, e1p), (a2, e2p), (d, d_p), (x, xp), (z, zp) = _sweep_args(K, (origins, (3,)), (e1s, (3,)), (e2s, (3,)), (displacements, (M, 3)), (xs, (n,)), (zs, (n,)))
    out = _out(K1 * M * n * n)
    fld = _out(2 * K1 * M * n * n) if want_field else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_through_focus_sweep(res_handle, int(detector), K, op, e1p, e2p, d_p, M, xp, zp, n, out.ctypes.data_as(dp),
                                               fld.ctypes.data_as(dp) if want_field else None, C.byref(ms)), "bmo_psf_through_focus_sweep")
    field = np.ascontiguousarray((fld[0::2] + 1j * fld[1::2]).reshape(K1, M, n, n).transpose(0, 1, 3, 2))[:K] if want_field else None
    return np.ascontiguousarray(out.reshape(K1, M, n, n).transpose(0, 1, 3, 2))[:K], field, ms.value


def psf_geo_otf_sweep(res_handle, detector, n_configs, origins, e1s, e2s, axes, offsets, freqs, centers=None):
    """bmo_psf_geo_otf_sweep: axes [K, 3], offsets [K, M] (or one list for all), freqs [nf, 2] for all configurations, centers None or
    [K, M, 2].  Returns (mtf [K, M, nf], otf [K, M, nf] complex, sums [K, M], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    K1 = max(K, 1)
    off = _sweep_planes(K, offsets)
    fq = _freqs(freqs)
    M, nf = off.shape[1], len(fq)
    (o, op), (a1, e1p), (a2, e2p), (ax, axp), (cen, cenp) = _sweep_args(K, (origins, (3,)), (e1s, (3,)), (e2s, (3,)), (axes, (3,)), (centers, (M, 2)))
    otf, mtf, sums = _out((K1, M, nf, 2)), _out((K1, M, nf)), _out((K1, M))
    ms = C.c_double()
    check(lib, lib.bmo_psf_geo_otf_sweep(res_handle, int(detector), K, op, e1p, e2p, axp, off.ctypes.data_as(dp), cenp, M, fq.ctypes.data_as(dp), nf,
                                         otf.ctypes.data_as(dp), mtf.ctypes.data_as(dp), sums.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_geo_otf_sweep")
    return mtf[:K], (otf[..., 0] + 1j * otf[..., 1])[:K], sums[:K], ms.value


def psf_otf_sweep(res_handle, detector, n_configs, origins, e1s, e2s, displacements, xs, zs, freqs, want_intensity=False):
    """bmo_psf_otf_sweep: the arguments of psf_through_focus_sweep and freqs [nf, 2] for all configurations.  Returns (mtf [K, M, nf],
    otf [K, M, nf] complex, sums [K, M], I[K, M, n, n] indexed [c, m, i, j] or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    K1 = max(K, 1)
    n = np.asarray(xs).shape[-1]
    M = np.asarray(displacements).size // (3 * K1)
    fq = _freqs(freqs)
    nf = len(fq)
    (o, op), (a1, e1p), (a2, e2p), (d, d_p), (x, xp), (z, zp) = _sweep_args(K, (origins, (3,)), (e1s, (3,)), (e2s, (3,)), (displacements, (M, 3)), (xs, (n,)), (zs, (n,)))
    otf, mtf, sums = _out((K1, M, nf, 2)), _out((K1, M, nf)), _out((K1, M))
    img = _out(K1 * M * n * n) if want_intensity else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_otf_sweep(res_handle, int(detector), K, op, e1p, e2p, d_p, M, xp, zp, n, fq.ctypes.data_as(dp), nf, otf.ctypes.data_as(dp),
                                     mtf.ctypes.data_as(dp), sums.ctypes.data_as(dp), img.ctypes.data_as(dp) if want_intensity else None, C.byref(ms)),
          "bmo_psf_otf_sweep")
    I = np.ascontiguousarray(img.reshape(K1, M, n, n).transpose(0, 1, 3, 2))[:K] if want_intensity else None
    return mtf[:K], (otf[..., 0] + 1j * otf[..., 1])[:K], sums[:K], I, ms.value


class PsfBands:
    """A bmo_psf_bands handle: the PSF rows of one buffer split by wave number into band-contiguous ranges on the device.  `ks` [B] the
    bands' wave numbers, `counts` int64 [B] their rows, `unmatched` the rows of no band, `device` the ordinal the rows lie on;
    rows(b) -> (device pointer, count) to hand to any read-out as hits_device_ptr / n_hits with device=self.device.  A context manager;
    close() frees the device rows."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle
        nb, n_rows, unmatched, device = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int32()
        check(lib, lib.bmo_psf_bands_info(handle, C.byref(nb), C.byref(n_rows), C.byref(unmatched), C.byref(device)), "bmo_psf_bands_info")
        self.n_rows, self.unmatched, self.device = n_rows.value, unmatched.value, device.value
        self.ks, self.counts, self._ptrs = _out(nb.value), _out(nb.value, dtype=np.int64), []  # (filled band by band below)
        for b in range(nb.value):
            k, p, cnt = C.c_double(), C.POINTER(C.c_double)(), C.c_int64()
            check(lib, lib.bmo_psf_bands_get(handle, b, C.byref(k), C.byref(p), C.byref(cnt)), "bmo_psf_bands_get")
            self.ks[b], self.counts[b] = k.value, cnt.value
            self._ptrs.append(C.cast(p, C.c_void_p).value or 0)

    def __len__(self):
        return len(self.ks)

    def rows(self, b):
        if self.handle is None:
            raise ValueError("PsfBands: the handle is closed")
        if not 0 <= int(b) < len(self.ks):
            raise IndexError("PsfBands.rows: band index out of range")
        return self._ptrs[int(b)], int(self.counts[int(b)])

    def close(self):
        if self.handle is not None:
            self.lib.bmo_psf_bands_free(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def psf_bands(hits, ks=None, device=0, hits_device_ptr=None, n_hits=None, want_ms=False):
    """bmo_psf_bands_create: the rows split by wave number (column 8, a plain == compare), stably, on the device.  ks None: the bands are the
    distinct wave numbers of the rows, ascending; otherwise exactly the bands `ks`, in that order.  `hits` is a host [H, 9] array, or pass
    `hits_device_ptr` + `n_hits` for rows resident on `device`.  Returns a PsfBands (with want_ms: (PsfBands, kernel_ms))."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    kk = None if ks is None else np.ascontiguousarray(np.asarray(ks, dtype=np.float64).reshape(-1))
    h = C.c_void_p()
    ms = C.c_double()
    check(lib, lib.bmo_psf_bands_create(hp, nh, on_dev, int(device), None if kk is None else kk.ctypes.data_as(dp), 0 if kk is None else len(kk), C.byref(h),
                                        C.byref(ms)), "bmo_psf_bands_create")
    bands = PsfBands(lib, h)
    return (bands, ms.value) if want_ms else bands


def _poly_args(bands, origin, e1, e2, displacements, xs, zs, coeffs):
    if not isinstance(bands, PsfBands) or bands.handle is None:
        raise ValueError("bands must be an open PsfBands")
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    d = np.ascontiguousarray(np.asarray(displacements, dtype=np.float64).reshape(-1, 3))
    x, z = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(zs, dtype=np.float64)
    if len(z) != len(x):
        raise ValueError("xs and zs must have the same length")
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).reshape(-1))
    if len(c) != len(bands):
        raise ValueError("coeffs must hold one coefficient per band (%d), got %d" % (len(bands), len(c)))
    return o, a1, a2, d, x, z, c


def psf_poly_through_focus(bands, origin, e1, e2, displacements, xs, zs, coeffs, want_bands=False):
    """bmo_psf_poly_through_focus: the incoherent sum ((c_0 I_0 + c_1 I_1) + ...) of the bands' through-focus stacks, I_b what
    psf_through_focus returns for band b's rows.  Returns (I[M, n, n] indexed [m, i, j], I_b [B, M, n, n] or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2, d, x, z, c = _poly_args(bands, origin, e1, e2, displacements, xs, zs, coeffs)
    n, M, B = len(x), len(d), len(bands)
    out = _out(M * n * n)
    per = _out(B * M * n * n) if want_bands else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_poly_through_focus(bands.handle, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), d.ctypes.data_as(dp), M,
                                              x.ctypes.data_as(dp), z.ctypes.data_as(dp), n, c.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                              per.ctypes.data_as(dp) if want_bands else None, C.byref(ms)), "bmo_psf_poly_through_focus")
    I_b = np.ascontiguousarray(per.reshape(B, M, n, n).transpose(0, 1, 3, 2)) if want_bands else None
    return np.ascontiguousarray(out.reshape(M, n, n).transpose(0, 2, 1)), I_b, ms.value


def psf_poly_otf(bands, origin, e1, e2, displacements, xs, zs, coeffs, freqs, want_intensity=False):
    """bmo_psf_poly_otf: the transform of the combined stack of psf_poly_through_focus (kept on the device) at the frequencies `freqs`
    [nf, 2] (cycles per metre).  Returns (mtf [M, nf], otf [M, nf] complex, sums [M], I[M, n, n] indexed [m, i, j] or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2, d, x, z, c = _poly_args(bands, origin, e1, e2, displacements, xs, zs, coeffs)
    fq = _freqs(freqs)
    n, M, nf = len(x), len(d), len(fq)
    otf, mtf, sums = _out((M, nf, 2)), _out((M, nf)), _out(M)
    img = _out(M * n * n) if want_intensity else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_poly_otf(bands.handle, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), d.ctypes.data_as(dp), M, x.ctypes.data_as(dp),
                                    z.ctypes.data_as(dp), n, c.ctypes.data_as(dp), fq.ctypes.data_as(dp), nf, otf.ctypes.data_as(dp), mtf.ctypes.data_as(dp),
                                    sums.ctypes.data_as(dp), img.ctypes.data_as(dp) if want_intensity else None, C.byref(ms)), "bmo_psf_poly_otf")
    I = np.ascontiguousarray(img.reshape(M, n, n).transpose(0, 2, 1)) if want_intensity else None
    return mtf, otf[..., 0] + 1j * otf[..., 1], sums, I, ms.value


EE_SHAPES = {"circle": 0, "square": 1}


def _ee_shape(shape):
    """The shape code of the encircled-energy entries: "circle" / 0, "square" / 1 (another integer goes through for the library to refuse)."""
    if isinstance(shape, str):
        if shape not in EE_SHAPES:
            raise ValueError('encircled energy: shape must be "circle" or "square"')
        return EE_SHAPES[shape]
    return int(shape)


def _radii(radii):
    return np.ascontiguousarray(np.asarray(radii, dtype=np.float64).reshape(-1))


def spot_ee(rows, center, radii, shape="circle", device=0, rows_device_ptr=None, n_rows=None, row_cols=9):
    """bmo_spot_ee: the number of rows [n, 2..9] (x in column 0, z in column 1) inside a circle (r2 <= R * R) or a square (|ax| <= R and
    |az| <= R) of half-size R about `center`, for every R of `radii` (any order).  Returns (inside int64 [n_radii], kernel_ms).  `rows` is
    a host array, or pass `rows_device_ptr` + `n_rows` + `row_cols` for rows already resident on `device`."""
    lib = load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    rp, n, cols, on_dev, keep = _spot_rows(rows, rows_device_ptr, n_rows, row_cols)
    c = np.ascontiguousarray(center, dtype=np.float64).reshape(2)
    r = _radii(radii)
    inside = _out(len(r), dtype=np.int64)
    ms = C.c_double()
    check(lib, lib.bmo_spot_ee(rp, n, cols, on_dev, c.ctypes.data_as(dp), _ee_shape(shape), r.ctypes.data_as(dp), len(r), int(device), inside.ctypes.data_as(ip),
                               C.byref(ms)), "bmo_spot_ee")
    return inside, ms.value


def spot_ee_sweep(res_handle, detector, n_configs, centers, radii, shape="circle"):
    """bmo_spot_ee_sweep on the result handle `res_handle`: centers [K, 2] (or one centre for all).  Returns (inside int64 [K, n_radii],
    n_rows int64 [K], kernel_ms); configuration c equals spot_ee on its rows."""
    lib = load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    K = int(n_configs)
    K1 = max(K, 1)
    c = _per_config(centers, K1, 2)
    r = _radii(radii)
    inside, n_rows = _out((K1, len(r)), dtype=np.int64), _out(K1, dtype=np.int64)
    ms = C.c_double()
    check(lib, lib.bmo_spot_ee_sweep(res_handle, int(detector), K, c.ctypes.data_as(dp), _ee_shape(shape), r.ctypes.data_as(dp), len(r), inside.ctypes.data_as(ip),
                                     n_rows.ctypes.data_as(ip), C.byref(ms)), "bmo_spot_ee_sweep")
    return inside[:K], n_rows[:K], ms.value


def psf_geo_ee(hits, origin, e1, e2, axis, offsets, radii, centers=None, shape="circle", device=0, hits_device_ptr=None, n_hits=None, want_count=True):
    """bmo_psf_geo_ee: the proj-weighted share of the rows, propagated to the detector plane moved by offsets[m] * axis, inside a circle or a
    square of half-size R about centers[m] ([M, 2]; None: the plane's origin), for every R of `radii`.  Returns (ee [M, nr], energy [M, nr],
    count int64 [M, nr] or None, sums [M], kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2, ax = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2, axis))
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.float64).reshape(-1))
    r = _radii(radii)
    M, nr = len(off), len(r)
    cen = None if centers is None else np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(M, 2))
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    ee, energy, sums = _out((M, nr)), _out((M, nr)), _out(M)
    count = _out((M, nr), dtype=np.int64) if want_count else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_geo_ee(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), ax.ctypes.data_as(dp), off.ctypes.data_as(dp),
                                  None if cen is None else cen.ctypes.data_as(dp), M, _ee_shape(shape), r.ctypes.data_as(dp), nr, int(device), ee.ctypes.data_as(dp),
                                  energy.ctypes.data_as(dp), count.ctypes.data_as(C.POINTER(C.c_int64)) if want_count else None, sums.ctypes.data_as(dp),
                                  C.byref(ms)), "bmo_psf_geo_ee")
    return ee, energy, count, sums, ms.value


def psf_ee(hits, origin, e1, e2, displacements, xs, zs, radii, centers=None, shape="circle", device=0, hits_device_ptr=None, n_hits=None, want_intensity=False):
    """bmo_psf_ee: the share of the pixel sums of the through-focus stack (psf_through_focus of the same arguments, kept on the device) inside
    a circle or a square of half-size R about centers[m] ([M, 2] in the coordinates of xs and zs; None: each image's intensity centroid),
    for every R of `radii`.  Returns (ee [M, nr], energy [M, nr], sums [M], centers [M, 2] as used, I[M, n, n] indexed [m, i, j] or None,
    kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    d = np.ascontiguousarray(np.asarray(displacements, dtype=np.float64).reshape(-1, 3))
    x, z = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(zs, dtype=np.float64)
    r = _radii(radii)
    n, M, nr = len(x), len(d), len(r)
    if len(z) != n:
        raise ValueError("xs and zs must have the same length")
    cen = None if centers is None else np.ascontiguousarray(np.asarray(centers, dtype=np.float64).reshape(M, 2))
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    ee, energy, sums, cout = _out((M, nr)), _out((M, nr)), _out(M), _out((M, 2))
    img = _out(M * n * n) if want_intensity else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_ee(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), d.ctypes.data_as(dp), M, x.ctypes.data_as(dp),
                              z.ctypes.data_as(dp), n, None if cen is None else cen.ctypes.data_as(dp), _ee_shape(shape), r.ctypes.data_as(dp), nr, int(device),
                              ee.ctypes.data_as(dp), energy.ctypes.data_as(dp), sums.ctypes.data_as(dp), cout.ctypes.data_as(dp),
                              img.ctypes.data_as(dp) if want_intensity else None, C.byref(ms)), "bmo_psf_ee")
    I = np.ascontiguousarray(img.reshape(M, n, n).transpose(0, 2, 1)) if want_intensity else None
    return ee, energy, sums, cout, I, ms.value


def zernike_sizes(order):
    """(J, E): the terms up to radial order `order`, and the entries of the packed augmented Gram matrix."""
    J = (int(order) + 1) * (int(order) + 2) // 2
    return J, (J + 1) * (J + 2) // 2


def psf_zernike(hits, origin, e1, e2, order=4, ref=None, pupil=None, device=0, hits_device_ptr=None, n_hits=None, want_gram=False):
    """bmo_psf_zernike: the least-squares Zernike coefficients (OSA/ANSI order, metres) of the wavefront of PSF rows at the detector pose
    (origin, e1, e2), four passes on the device.  ref: the reference point (x, z), None for the centroid; pupil: (U0, V0, RHO) in direction
    cosines, None for the proj-weighted centre and the largest radius of the rows.  `hits` is a host [H, 9] array, or pass
    `hits_device_ptr` + `n_hits` for resident rows.  Returns (coef [J], info [13] at the ZERN_* columns, gram or None, kernel_ms)."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    r = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64).reshape(2)
    q = None if pupil is None else np.ascontiguousarray(pupil, dtype=np.float64).reshape(3)
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    J, E = zernike_sizes(min(max(int(order), 0), ZERN_MAX_ORDER))
    coef, info = _out(J), _out(ZERN_INFO_N)
    gram = _out(E) if want_gram else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_zernike(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), None if r is None else r.ctypes.data_as(dp),
                                   None if q is None else q.ctypes.data_as(dp), int(order), int(device), coef.ctypes.data_as(dp), info.ctypes.data_as(dp),
                                   gram.ctypes.data_as(dp) if want_gram else None, C.byref(ms)), "bmo_psf_zernike")
    return coef, info, gram, ms.value


def psf_zernike_sweep(res_handle, detector, n_configs, origins, e1s, e2s, order=4, ref=None, pupil=None, want_gram=False):
    """bmo_psf_zernike_sweep on the result handle `res_handle`: origins / e1s / e2s [K, 3]; ref None, one (x, z) for all or [K, 2]; pupil
    None, one (U0, V0, RHO) for all or [K, 3].  Returns (coef [K, J], info [K, 13], gram [K, E] or None, kernel_ms); row c equals
    psf_zernike on the rows of configuration c bit for bit."""
    lib = load_engine()
    dp = C.POINTER(C.c_double)
    K = int(n_configs)
    K1 = max(K, 1)
    o, a1, a2 = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(K1, 3)) for v in (origins, e1s, e2s))
    r, q = _per_config(ref, K1, 2), _per_config(pupil, K1, 3)
    J, E = zernike_sizes(min(max(int(order), 0), ZERN_MAX_ORDER))
    coef, info = _out((K1, J)), _out((K1, ZERN_INFO_N))
    gram = _out((K1, E)) if want_gram else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_zernike_sweep(res_handle, int(detector), K, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp),
                                         None if r is None else r.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), int(order),
                                         coef.ctypes.data_as(dp), info.ctypes.data_as(dp), gram.ctypes.data_as(dp) if want_gram else None, C.byref(ms)),
          "bmo_psf_zernike_sweep")
    return coef[:K], info[:K], None if gram is None else gram[:K], ms.value


def _opd_maps(a, K, n):
    """[K, n * n] with bin (i, j) at i + n * j -> [K, n, n] indexed [c, i, j]"""
    return np.ascontiguousarray(a.reshape(K, n, n, *a.shape[2:]).swapaxes(1, 2))


def psf_opd_map(hits, origin, e1, e2, n=64, order=0, coef=None, ref=None, pupil=None, device=0, hits_device_ptr=None, n_hits=None, want_raw=False):
    """bmo_psf_opd_map: the wavefront of PSF rows at the detector pose (origin, e1, e2) less the Zernike surface `coef` ([J] at `order`,
    metres; None with order 0: nothing removed), as the proj-weighted mean per bin of an n x n grid over the pupil square, binned on the
    device with integer sums.  ref, pupil, `hits` / `hits_device_ptr`: as psf_zernike.  Returns (opd [n, n] indexed [i, j], weight [n, n],
    count int64 [n, n], info [20] at the OPD_* columns, raw int64 [n, n, 2] of (Q, P) or None, kernel_ms)."""
    lib = load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    o, a1, a2 = (np.ascontiguousarray(v, dtype=np.float64).reshape(3) for v in (origin, e1, e2))
    r = None if ref is None else np.ascontiguousarray(ref, dtype=np.float64).reshape(2)
    q = None if pupil is None else np.ascontiguousarray(pupil, dtype=np.float64).reshape(3)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
    if cf is not None and len(cf) != zernike_sizes(order)[0]:
        raise ValueError("psf_opd_map: coef must have the (order + 1)(order + 2) / 2 terms of `order`")
    hp, nh, on_dev, keep = _psf_rows(hits, hits_device_ptr, n_hits)
    nb = min(max(int(n), 1), OPD_MAX_N)
    opd, weight, count, info = _out((1, nb * nb)), _out((1, nb * nb)), _out((1, nb * nb), dtype=np.int64), _out(OPD_INFO_N)
    raw = _out((1, nb * nb, 2), dtype=np.int64) if want_raw else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_opd_map(hp, nh, on_dev, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp), None if r is None else r.ctypes.data_as(dp),
                                   None if q is None else q.ctypes.data_as(dp), int(order), None if cf is None else cf.ctypes.data_as(dp), int(n), int(device),
                                   opd.ctypes.data_as(dp), weight.ctypes.data_as(dp), count.ctypes.data_as(ip), raw.ctypes.data_as(ip) if want_raw else None,
                                   info.ctypes.data_as(dp), C.byref(ms)), "bmo_psf_opd_map")
    return _opd_maps(opd, 1, nb)[0], _opd_maps(weight, 1, nb)[0], _opd_maps(count, 1, nb)[0], info, _opd_maps(raw, 1, nb)[0] if want_raw else None, ms.value


def psf_opd_map_sweep(res_handle, detector, n_configs, origins, e1s, e2s, n=64, order=0, coef=None, ref=None, pupil=None, want_raw=False):
    """bmo_psf_opd_map_sweep on the result handle `res_handle`: origins / e1s / e2s [K, 3]; ref, pupil as psf_zernike_sweep; coef None
    (order 0), one [J] for all or [K, J].  Returns (opd [K, n, n] indexed [c, i, j], weight, count int64, info [K, 20], raw [K, n, n, 2] or
    None, kernel_ms); configuration c equals psf_opd_map on its rows bit for bit."""
    lib = load_engine()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    K = int(n_configs)
    K1 = max(K, 1)
    o, a1, a2 = (np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(K1, 3)) for v in (origins, e1s, e2s))
    r, q = _per_config(ref, K1, 2), _per_config(pupil, K1, 3)
    cf = _per_config(coef, K1, zernike_sizes(min(max(int(order), 0), ZERN_MAX_ORDER))[0])
    nb = min(max(int(n), 1), OPD_MAX_N)
    opd, weight, count, info = _out((K1, nb * nb)), _out((K1, nb * nb)), _out((K1, nb * nb), dtype=np.int64), _out((K1, OPD_INFO_N))
    raw = _out((K1, nb * nb, 2), dtype=np.int64) if want_raw else None
    ms = C.c_double()
    check(lib, lib.bmo_psf_opd_map_sweep(res_handle, int(detector), K, o.ctypes.data_as(dp), a1.ctypes.data_as(dp), a2.ctypes.data_as(dp),
                                         None if r is None else r.ctypes.data_as(dp), None if q is None else q.ctypes.data_as(dp), int(order),
                                         None if cf is None else cf.ctypes.data_as(dp), int(n), opd.ctypes.data_as(dp), weight.ctypes.data_as(dp),
                                         count.ctypes.data_as(ip), raw.ctypes.data_as(ip) if want_raw else None, info.ctypes.data_as(dp), C.byref(ms)),
          "bmo_psf_opd_map_sweep")
    return (_opd_maps(opd, K1, nb)[:K], _opd_maps(weight, K1, nb)[:K], _opd_maps(count, K1, nb)[:K], info[:K], _opd_maps(raw, K1, nb)[:K] if want_raw else None,
            ms.value)
