"""System container, scene compiler and the `solve_system` entry point.

Mirrors src/System.jl: `System(objects)` (:10-21) and
`solve_system!(system, beam|group; r_max=100)` (:444-468).  The scene is flattened in
`Leaves` order into the tables of include/bmo.h and handed to the HIP engine through the
C ABI; the beam trees are rebuilt from the engine's result tables in reference order.
"""
import ctypes as C
import math

import numpy as np

from . import abi
from . import beams as bm
from . import components as cp
from . import shapes as sh
from . import linalg as la

# miss-cull inflation of bounding spheres (see DESIGN.md "miss cull")
_BS_REL, _BS_ABS = 1e-6, 1e-6


class System:
    """src/System.jl:10-21"""

    def __init__(self, objects):
        self.objects_tree = list(objects) if isinstance(objects, (list, tuple)) else [objects]

    def objects(self):
        return cp.leaves(self.objects_tree)


StaticSystem = System  # src/System.jl:38-45: same tracing semantics


class CompiledScene:
    """Flat tables + the ctypes descriptor that points into them (kept alive together)."""

    def __init__(self, system, lambdas, cull=True, consts=None, mesh_bvh=True):
        # mesh_bvh=False: every mesh keeps the brute-force face loop (BMO_SHAPE_FLAG_NO_BVH); True: meshes of
        # sh.MESH_BVH_MIN_FACES faces or more are traced through a BVH with the same results, bit for bit
        objs = system.objects() if isinstance(system, System) else cp.leaves(system)
        self.leaf_objects = objs
        self.lambdas = np.array(sorted(set(float(l) for l in lambdas)), dtype=np.float64)
        self.shape_list = []   # python shape per shape id
        self._shape_ids = {}
        shapes, children, tris, coefs = [], [], [], []
        media, media_ids = [], {}

        def medium_of(fn):
            key = id(fn)
            if key not in media_ids:
                media_ids[key] = len(media)
                media.append([float(fn(l)) for l in self.lambdas])
            return media_ids[key]

        slope = {}  # shape id -> K of "sdf >= dist / K" (1 for exact sdfs; None: no bound, never culled)

        def add_shape(s):
            if id(s) in self._shape_ids:
                return self._shape_ids[id(s)]
            rec = abi.Shape()
            sid = len(shapes)
            shapes.append(rec)
            self.shape_list.append(s)
            self._shape_ids[id(s)] = sid
            rec.kind = s.kind
            rec.child_begin = rec.child_count = rec.tri_begin = rec.tri_count = rec.flags = 0
            rec.pos[:] = list(s.pos)
            rec.dir[:] = list(np.asarray(s.dir, dtype=np.float64).reshape(9))
            tdir = s.tdir if hasattr(s, "tdir") else np.asarray(s.dir).T
            rec.tdir[:] = list(np.asarray(tdir, dtype=np.float64).reshape(9))
            p = list(s.params()) if hasattr(s, "params") else []
            rec.p[:] = p + [0.0] * (abi.NPARAM - len(p))
            if s.kind == sh.K_MESH:
                t = s.triangles()
                rec.tri_begin = len(tris)
                rec.tri_count = len(t)
                tris.extend(t)
                if not mesh_bvh:
                    rec.flags |= sh.FLAG_NO_BVH
                v = s.vertices
                c = (v.min(axis=0) + v.max(axis=0)) / 2
                r = float(np.sqrt(((v - c) ** 2).sum(axis=1)).max())
            elif s.kind in (sh.K_UNION, sh.K_MENISCUS):
                ids = [add_shape(ch) for ch in s.sdfs]
                rec.child_begin = len(children)
                rec.child_count = len(ids)
                children.extend(ids)
                c, r = s.world_bound()
                if any(shapes[i].flags & sh.FLAG_INEXACT for i in ids):
                    rec.flags |= sh.FLAG_INEXACT
                ks = [slope[i] for i in (ids[:2] if s.kind == sh.K_MENISCUS else ids)]  # min over children: the weakest bound holds
                slope[sid] = None if any(k is None for k in ks) else max(ks)
            elif s.kind in (sh.K_ASPH_CONVEX, sh.K_ASPH_CONCAVE, sh.K_ACYL_CONVEX, sh.K_ACYL_CONCAVE):
                rec.child_begin = len(coefs)
                rec.child_count = len(s.coefficients)
                coefs.extend(s.coefficients)
                rec.flags |= sh.FLAG_INEXACT
                c, r = s.world_bound()
                slope[sid] = s.slope_bound()
            else:
                c, r = s.world_bound()
            K = slope.setdefault(sid, 1.0)
            if cull and K is not None:
                # outside the inflated sphere dist(p, solid) >= K * (r * 1e-6 + 1 um), hence sdf(p) >= r * 1e-6 + 1 um: the
                # reference's start classification is "outside" (> 1e-9) and its hit test (< 1e-10) can never fire
                rec.bs_center[:] = list(c)
                rec.bs_radius = r + K * (r * _BS_REL + _BS_ABS)
            else:
                rec.bs_center[:] = [0.0, 0.0, 0.0]
                rec.bs_radius = -1.0
            return sid

        objects = []
        self.detectors = []
        for o in objs:
            rec = abi.Object()
            rec.kind = o.kind
            rec.shape[:] = [-1, -1, -1]
            rec.medium[:] = [-1, -1]
            rec.detector = -1
            rec.reflectance = rec.transmittance = rec.cutoff = 0.0
            parts = o.parts()
            for k, s in enumerate(parts):
                rec.shape[k] = add_shape(s)
            if o.kind == cp.O_REFRACTIVE:
                rec.medium[0] = medium_of(o.n)
            elif o.kind == cp.O_DOUBLET:
                rec.medium[0] = medium_of(o.front.n)
                rec.medium[1] = medium_of(o.back.n)
            elif o.kind == cp.O_THIN_BS:
                rec.reflectance, rec.transmittance = o.reflectance, o.transmittance
            elif o.kind == cp.O_PLATE_BS:
                rec.medium[0] = medium_of(o.substrate.n)
                rec.reflectance, rec.transmittance = o.coating.reflectance, o.coating.transmittance
            elif o.kind == cp.O_CUBE_BS:
                rec.medium[0] = medium_of(o.front.n)
                rec.medium[1] = medium_of(o.back.n)
                rec.reflectance, rec.transmittance = o.coating.reflectance, o.coating.transmittance
            elif o.kind in (cp.O_SPOT, cp.O_PSF, cp.O_PHOTODETECTOR):
                rec.detector = len(self.detectors)
                self.detectors.append(o)
            elif o.kind == cp.O_POLARIZER:
                rec.cutoff = o.cutoff
                j = np.asarray(o.jones, dtype=np.complex128).reshape(9)
                rec.jones[:] = [x for z in j for x in (z.real, z.imag)]
            objects.append(rec)

        self.n_objects = len(objects)
        self._objects = (abi.Object * max(1, len(objects)))(*objects)
        self._shapes = (abi.Shape * max(1, len(shapes)))(*shapes)
        self._children = np.array(children if children else [0], dtype=np.int32)
        self._tris = np.array(tris if tris else [[0.0] * 9], dtype=np.float64).reshape(-1)
        self._ntab = np.array(media if media else [[1.0] * max(1, len(self.lambdas))], dtype=np.float64).reshape(-1)
        self._coefs = np.array(coefs if coefs else [0.0], dtype=np.float64)
        d = abi.SceneDesc()
        d.abi_version = abi.ABI_VERSION
        d.n_objects, d.n_shapes, d.n_children = len(objects), len(shapes), len(children)
        d.n_tris, d.n_media, d.n_lambda, d.n_detectors = len(tris), len(media), len(self.lambdas), len(self.detectors)
        d.objects = C.cast(self._objects, C.POINTER(abi.Object))
        d.shapes = C.cast(self._shapes, C.POINTER(abi.Shape))
        d.children = self._children.ctypes.data_as(C.POINTER(C.c_int32))
        d.tris = self._tris.ctypes.data_as(C.POINTER(C.c_double))
        d.n_table = self._ntab.ctypes.data_as(C.POINTER(C.c_double))
        d.lambdas = self.lambdas.ctypes.data_as(C.POINTER(C.c_double))
        d.coefs = self._coefs.ctypes.data_as(C.POINTER(C.c_double))
        d.n_coefs = len(coefs)
        k = dict(eps_srf=1e-9, eps_ray=1e-10, eps_ins=1.0, mt_keps=1e-9, mt_leps=1e-9, grad_h=1e-8, march_iters=1000)
        k.update(consts or {})
        for name, val in k.items():
            setattr(d, name, val)
        self.desc = d

    def shape_id(self, shape):
        return self._shape_ids[id(shape)]

    def lambda_index(self, lams):
        lams = np.asarray(lams, dtype=np.float64)
        idx = np.searchsorted(self.lambdas, lams)
        if np.any(idx >= len(self.lambdas)) or np.any(self.lambdas[np.minimum(idx, len(self.lambdas) - 1)] != lams):
            raise KeyError("wavelength not in the compiled lambda table")
        return idx.astype(np.int32)


class _SceneHandle:
    """bmo_scene of a CompiledScene for the host-side entries (no GPU needed)."""

    def __init__(self, scene):
        self.lib = abi.load_engine()
        self.handle = C.c_void_p()
        abi.check(self.lib, self.lib.bmo_scene_create(C.byref(scene.desc), C.byref(self.handle)), "bmo_scene_create")

    def __del__(self):
        if getattr(self, "handle", None):
            self.lib.bmo_scene_destroy(self.handle)


def mesh_bvh_stats(scene):
    """{shape id: (n_nodes, depth, max_leaf)} of the BVHs the library builds for the mesh shapes of a CompiledScene
    (n_nodes = 0: that mesh is traced by brute force)."""
    h = _SceneHandle(scene)
    out = {}
    for sid, s in enumerate(scene.shape_list):
        if s.kind != sh.K_MESH:
            continue
        n, d, m = C.c_int32(), C.c_int32(), C.c_int32()
        abi.check(h.lib, h.lib.bmo_scene_mesh_bvh(h.handle, sid, C.byref(n), C.byref(d), C.byref(m)), "bmo_scene_mesh_bvh")
        out[sid] = (n.value, d.value, m.value)
    return out


def mesh_nearest_host(scene, shape_id, pos, dir):
    """intersect3d(mesh, ray) of one mesh shape for rays pos / dir (n x 3) as the engine's lane code computes it, on the host
    (bmo_mesh_nearest_host): (t, face) arrays, t = +Inf and face = -1 for a miss."""
    h = _SceneHandle(scene)
    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    dir = np.ascontiguousarray(dir, dtype=np.float64).reshape(-1, 3)
    n = len(pos)
    assert dir.shape == pos.shape
    t = np.empty(n, dtype=np.float64)
    fid = np.empty(n, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    abi.check(h.lib, h.lib.bmo_mesh_nearest_host(h.handle, int(shape_id), n, pos.ctypes.data_as(dp), dir.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                                 fid.ctypes.data_as(C.POINTER(C.c_int32))), "bmo_mesh_nearest_host")
    return t, fid


def make_batch(scene, bundle):
    """bmo_ray_batch for a RayBundle; returns (batch, keepalive)."""
    li = scene.lambda_index(bundle.lambdas)
    planes = np.ascontiguousarray(bundle.planes, dtype=np.float64)
    b = abi.RayBatch()
    b.n = bundle.n
    b.kind = bundle.kind
    b.n_planes = planes.shape[0]
    b.planes = planes.ctypes.data_as(C.POINTER(C.c_double))
    b.lambda_idx = li.ctypes.data_as(C.POINTER(C.c_int32))
    return b, (planes, li)


class Engine:
    """Thin RAII wrapper over the C ABI for one compiled scene."""

    def __init__(self, scene, device=0, max_beams=0):
        self.lib = abi.load_engine()
        self.scene = scene
        self.device = device
        self.max_beams = max_beams  # bmo_trace_opts.max_beams: 0 = no limit (reference behaviour)
        self.handle = C.c_void_p()
        abi.check(self.lib, self.lib.bmo_scene_create(C.byref(scene.desc), C.byref(self.handle)), "bmo_scene_create")

    def close(self):
        if self.handle:
            self.lib.bmo_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def opts(self, r_max, record_segments=True):
        o = abi.TraceOpts()
        o.r_max, o.device, o.record_segments, o.max_beams = int(r_max), int(self.device), int(bool(record_segments)), int(self.max_beams)
        return o

    def trace(self, bundle, r_max=100):
        """bmo_trace: upload + trace + download; returns abi.TraceResult."""
        batch, keep = make_batch(self.scene, bundle)
        res = C.c_void_p()
        o = self.opts(r_max)
        abi.check(self.lib, self.lib.bmo_trace(self.handle, C.byref(batch), C.byref(o), C.byref(res)), "bmo_trace")
        try:
            v = abi.ResultView()
            abi.check(self.lib, self.lib.bmo_result_view(res, C.byref(v)), "bmo_result_view")
            out = abi.TraceResult(v)
            ms, tot, nl = C.c_double(), C.c_double(), C.c_int32()
            self.lib.bmo_result_timing(res, C.byref(ms), C.byref(tot), C.byref(nl))
            out.kernel_ms, out.total_ms, out.n_launches = ms.value, tot.value, nl.value
        finally:
            self.lib.bmo_result_free(res)
        return out

    # split form (inputs resident in HBM)
    def upload(self, bundle):
        batch, keep = make_batch(self.scene, bundle)
        h = C.c_void_p()
        abi.check(self.lib, self.lib.bmo_batch_upload(self.handle, C.byref(batch), self.device, C.byref(h)), "bmo_batch_upload")
        return h

    def free_batch(self, h):
        self.lib.bmo_batch_free(h)

    def trace_device(self, dev_batch, r_max=100, record_segments=True):
        res = C.c_void_p()
        o = self.opts(r_max, record_segments)
        abi.check(self.lib, self.lib.bmo_trace_device(self.handle, dev_batch, C.byref(o), C.byref(res)), "bmo_trace_device")
        return res

    def retrace_device(self, dev_batch, prev, r_max=100):
        """bmo_retrace_device: re-solve the batch of `prev` (a result handle) against this engine's scene."""
        res = C.c_void_p()
        o = self.opts(r_max)
        abi.check(self.lib, self.lib.bmo_retrace_device(self.handle, dev_batch, prev, C.byref(o), C.byref(res)), "bmo_retrace_device")
        return res

    def result_timing(self, res):
        ms, tot, nl = C.c_double(), C.c_double(), C.c_int32()
        abi.check(self.lib, self.lib.bmo_result_timing(res, C.byref(ms), C.byref(tot), C.byref(nl)), "bmo_result_timing")
        return ms.value, tot.value, nl.value

    def result_view(self, res, what=None):
        """bmo_result_view (the whole solution) or, with `what` (abi.VIEW_* mask), bmo_result_view_select."""
        v = abi.ResultView()
        if what is None:
            abi.check(self.lib, self.lib.bmo_result_view(res, C.byref(v)), "bmo_result_view")
        else:
            abi.check(self.lib, self.lib.bmo_result_view_select(res, int(what), C.byref(v)), "bmo_result_view_select")
        return abi.TraceResult(v)

    def result_device_hits(self, res, slot):
        p = C.POINTER(C.c_double)()
        n = C.c_int64()
        abi.check(self.lib, self.lib.bmo_result_device_hits(res, slot, C.byref(p), C.byref(n)), "bmo_result_device_hits")
        return C.cast(p, C.c_void_p).value or 0, n.value

    def result_copy_hits(self, res, slot, dst_device_ptr, max_hits):
        abi.check(self.lib, self.lib.bmo_result_copy_hits(res, slot, C.c_void_p(dst_device_ptr), max_hits), "bmo_result_copy_hits")

    def result_copy_hit_columns(self, res, slot, n_cols, dst_ptr, max_hits):
        """The leading n_cols columns of the ordered hit table of one detector, packed, into device or host memory."""
        abi.check(self.lib, self.lib.bmo_result_copy_hit_columns(res, slot, int(n_cols), C.c_void_p(dst_ptr), max_hits), "bmo_result_copy_hit_columns")

    def result_counts(self, res):
        """Per-detector hit counts without downloading anything."""
        return [self.result_device_hits(res, slot)[1] for slot in range(len(self.scene.detectors))]

    def result_size(self, res):
        """bmo_result_counts: (reference intersect3d calls, segments, beams, detector hits) without downloading the solution."""
        c, r, n, h = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        abi.check(self.lib, self.lib.bmo_result_counts(res, C.byref(c), C.byref(r), C.byref(n), C.byref(h)), "bmo_result_counts")
        return c.value, r.value, n.value, h.value

    def free_result(self, res):
        self.lib.bmo_result_free(res)


# ----------------------------------------------------------------------------------------
def _fill_beams(scene, res, roots):
    """Rebuild Beam / GaussianBeamlet trees in reference order from a TraceResult."""
    objs = scene.leaf_objects
    shapes = scene.shape_list
    kind = res.beam_kind
    nodes = [None] * res.n_nodes

    def make_rays(node, base, first):
        rays = []
        f, n = int(res.node_first_rec[node]), int(res.node_nseg[node])
        lam = res.node_aux[node, 3] if kind == bm.BEAM_GAUSSIAN else res.node_aux[node, 0]
        for r in range(f, f + n):
            P = res.rec[:, r]
            if kind == bm.BEAM_POLARIZED:
                ray = bm.PolarizedRay.__new__(bm.PolarizedRay)
                ray.E0 = P[11:17:2] + 1j * P[12:17:2]
            else:
                ray = bm.Ray.__new__(bm.Ray)
            ray.pos = P[base:base + 3].copy()
            ray.dir = P[base + 3:base + 6].copy()
            ray.n = float(P[base + 6])
            ray.lam = float(lam)
            t = float(P[base + 7])
            if np.isfinite(t):
                o, s = int(res.rec_obj[r]), int(res.rec_shape[r])
                ray.intersection = bm.Intersection(t, P[base + 8:base + 11].copy(), objs[o] if o >= 0 else None,
                                                   shapes[s] if s >= 0 else None)
            else:
                ray.intersection = None
            rays.append(ray)
        return rays

    for i in range(res.n_nodes):
        par = int(res.node_parent[i])
        if par < 0:
            b = roots[int(res.node_root[i])]
        elif kind == bm.BEAM_GAUSSIAN:
            b = bm.GaussianBeamlet(None, None, _parts=(bm.Beam.__new__(bm.Beam), bm.Beam.__new__(bm.Beam), bm.Beam.__new__(bm.Beam),
                                                       0.0, 0.0, 0j))
            for sub in (b.chief, b.waist, b.divergence):
                sub.parent, sub.children, sub.status = None, [], 0
        else:
            b = bm.Beam.__new__(bm.Beam)
            b.parent, b.children, b.status = None, [], 0
        nodes[i] = b
        b.status = int(res.node_status[i])
        b.children = []
        if kind == bm.BEAM_GAUSSIAN:
            b.chief.rays = make_rays(i, 0, True)
            b.waist.rays = make_rays(i, 11, False)
            b.divergence.rays = make_rays(i, 22, False)
            b.w0 = float(res.node_aux[i, 0])
            b.E0 = complex(res.node_aux[i, 1], res.node_aux[i, 2])
            b.lam = float(res.node_aux[i, 3])
        else:
            b.rays = make_rays(i, 0, True)
        if par >= 0:
            p = nodes[par]
            b.parent = p
            p.children.append(b)
            if kind == bm.BEAM_GAUSSIAN:
                b.chief.parent = p.chief  # parent! Gaussian.jl:113-117
    return nodes


class EngineSolution:
    """A solved batch that stays resident on the GPU (bmo_trace_result*), so that the next solve_system can retrace it."""

    def __init__(self, lib, handle, n_roots, kind):
        self.lib, self.handle, self.n_roots, self.kind = lib, handle, n_roots, kind

    def free(self):
        if self.handle:
            self.lib.bmo_result_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def gauss_parameters(self, node, zs):
        """bmo_gauss_parameters: rows (w, R, psi, w0) of beamlet `node` (result order) at the distances `zs` along the beam."""
        dp = C.POINTER(C.c_double)
        z = np.ascontiguousarray(zs, dtype=np.float64)
        out = abi._out((len(z), 4))
        abi.check(self.lib, self.lib.bmo_gauss_parameters(self.handle, int(node), z.ctypes.data_as(dp), len(z), out.ctypes.data_as(dp)), "bmo_gauss_parameters")
        return out

    def set_gauss_prefix(self, prefix_start, prefix_segs, opl_parent):
        """bmo_result_set_gauss_prefix: the earlier segments of continued beamlets ([n_roots + 1] starts, [24, total] planes, [n_roots] parent OPL)."""
        st = np.ascontiguousarray(prefix_start, dtype=np.int32)
        sg = np.ascontiguousarray(prefix_segs, dtype=np.float64)
        op = np.ascontiguousarray(opl_parent, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        abi.check(self.lib, self.lib.bmo_result_set_gauss_prefix(self.handle, len(op), st.ctypes.data_as(C.POINTER(C.c_int32)), sg.ctypes.data_as(dp),
                                                                 op.ctypes.data_as(dp)), "bmo_result_set_gauss_prefix")

    def photodetector_field(self, slot, position, orientation, xs, ys, field):
        """bmo_photodetector_field: adds the field of the beamlets recorded on detector `slot` to `field[i, j]` (in place)."""
        dp = C.POINTER(C.c_double)
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (position, np.asarray(orientation).reshape(9), xs, ys)]
        nx, ny = len(a[2]), len(a[3])
        buf = np.zeros(2 * nx * ny)  # (i, j) at [i + nx*j]
        ft = np.ascontiguousarray(field.T)
        buf[0::2], buf[1::2] = ft.real.reshape(-1), ft.imag.reshape(-1)
        ms = C.c_double()
        abi.check(self.lib, self.lib.bmo_photodetector_field(self.handle, int(slot), a[0].ctypes.data_as(dp), a[1].ctypes.data_as(dp),
                                                             a[2].ctypes.data_as(dp), a[3].ctypes.data_as(dp), nx, ny, buf.ctypes.data_as(dp),
                                                             C.byref(ms)), "bmo_photodetector_field")
        field[...] = (buf[0::2] + 1j * buf[1::2]).reshape(ny, nx).T
        return ms.value

    def spot_image(self, slot, window, nx, nz=None):
        """bmo_spot_image_sweep on the resident rows of Spotdetector slot `slot`: (counts int64 [nx, nz] indexed [i, j], outside), binned on
        window (x0, x1, z0, z1) by the floor rule of include/bmo.h."""
        img, outside, self.readout_ms = abi.spot_image_sweep(self.handle, slot, 1, window, nx, nz)
        return img[0], int(outside[0])

    def spot_stats(self, slot):
        """bmo_spot_stats_sweep on the resident rows of Spotdetector slot `slot`: the twelve statistics (abi.SPOT_* columns)."""
        st, self.readout_ms = abi.spot_stats_sweep(self.handle, slot, 1)
        return st[0]

    def psf_stats(self, slot, position, orientation, ref=None):
        """bmo_psf_stats_sweep on the resident rows of PSFDetector slot `slot` at the pose (position, orientation): the 21 wavefront statistics
        (abi.PSF_* columns) about ref = (x, z) in local coordinates (None: the centroid)."""
        o = np.asarray(orientation, dtype=np.float64)
        st, self.readout_ms = abi.psf_stats_sweep(self.handle, slot, 1, position, o[:, 0], o[:, 2], ref=ref)
        return st[0]

    def psf_zernike(self, slot, position, orientation, order=4, ref=None, pupil=None):
        """bmo_psf_zernike_sweep on the resident rows of PSFDetector slot `slot` at the pose (position, orientation): (coef [J], info [13] at
        the abi.ZERN_* columns) of the Zernike fit of the wavefront, as PSFDetector.zernike gives them from host rows."""
        o = np.asarray(orientation, dtype=np.float64)
        coef, info, _, self.readout_ms = abi.psf_zernike_sweep(self.handle, slot, 1, position, o[:, 0], o[:, 2], order=order, ref=ref, pupil=pupil)
        return coef[0], info[0]

    def psf_opd_map(self, slot, position, orientation, n=64, order=4, remove="tilt", ref=None, pupil=None):
        """The binned wavefront (OPD) map of the resident rows of PSFDetector slot `slot` at the pose (position, orientation)
        (bmo_psf_zernike_sweep, then bmo_psf_opd_map_sweep: no row leaves the device): (opd [n, n], weight, count, info [20], coef_removed)
        as PSFDetector.opd_map gives them from host rows."""
        o = np.asarray(orientation, dtype=np.float64)
        ms = []

        def zernike_fn(od, r, q):
            coef, info, _, t = abi.psf_zernike_sweep(self.handle, slot, 1, position, o[:, 0], o[:, 2], order=od, ref=r, pupil=q)
            ms.append(t)
            return coef[0], info[0]

        def map_fn(od, cf, r, q):
            opd, weight, count, info, _, t = abi.psf_opd_map_sweep(self.handle, slot, 1, position, o[:, 0], o[:, 2], n=n, order=od, coef=cf, ref=r, pupil=q)
            ms.append(t)
            return opd[0], weight[0], count[0], info[0]

        out = cp.psf_opd_map(zernike_fn, map_fn, n=n, order=order, remove=remove, ref=ref, pupil=pupil)
        self.readout_ms = float(sum(ms))
        return out

    def _psf_resident_rows(self, slot):
        """(device pointer, count, device) of the resident rows of PSFDetector slot `slot` (bmo_result_psf_rows: the library refuses a slot that
        is not a PSFDetector's and a GaussianBeamlet solution), for the single-call read-outs."""
        p, cnt, dev = C.POINTER(C.c_double)(), C.c_int64(), C.c_int32()
        abi.check(self.lib, self.lib.bmo_result_psf_rows(self.handle, int(slot), C.byref(p), C.byref(cnt), C.byref(dev)), "bmo_result_psf_rows")
        return C.cast(p, C.c_void_p).value or 0, cnt.value, dev.value

    def psf_focus_stats(self, slot, position, orientation, offsets, axis=None):
        """bmo_psf_focus_stats on the resident rows of PSFDetector slot `slot` at the pose (position, orientation): the twelve spot statistics
        (abi.FOCUS_* columns) of the rows propagated to the detector plane moved by each of `offsets` along `axis` (None: local y): [M, 12]."""
        o = np.asarray(orientation, dtype=np.float64)
        ptr, cnt, dev = self._psf_resident_rows(slot)
        st, self.readout_ms = abi.psf_focus_stats(None, position, o[:, 0], o[:, 2], o[:, 1] if axis is None else axis, offsets, device=dev,
                                                  hits_device_ptr=ptr, n_hits=cnt)
        return st

    def psf_through_focus(self, slot, position, orientation, offsets, n=100, axis=None, follow="centroid", window_plane=None, crop_factor=1.0):
        """The through-focus PSF stack of the resident rows of PSFDetector slot `slot` (bmo_psf_focus_stats, then bmo_psf_through_focus on the
        device pointer: no row leaves the device): (xs, zs, displacements, I[M, n, n], stats) as PSFDetector.through_focus gives them."""
        o = np.asarray(orientation, dtype=np.float64)
        ptr, cnt, dev = self._psf_resident_rows(slot)
        ms = [0.0, 0.0]

        def stats_fn(ax, off):
            st, ms[0] = abi.psf_focus_stats(None, position, o[:, 0], o[:, 2], ax, off, device=dev, hits_device_ptr=ptr, n_hits=cnt)
            return st

        def stack_fn(d, xs, zs):
            I, _, ms[1] = abi.psf_through_focus(None, position, o[:, 0], o[:, 2], d, xs, zs, device=dev, hits_device_ptr=ptr, n_hits=cnt)
            return I

        out = cp.psf_through_focus(stats_fn, stack_fn, o, offsets, n=n, axis=axis, follow=follow, window_plane=window_plane, crop_factor=crop_factor)
        self.readout_ms = ms[0] + ms[1]
        return out

    def psf_mtf(self, slot, position, orientation, freqs, offsets=(0.0,), kind="diffraction", n=None, half_width=None, axis=None, follow="centroid"):
        """The MTF of the resident rows of PSFDetector slot `slot` (bmo_psf_focus_stats, then bmo_psf_otf or bmo_psf_geo_otf on the device
        pointer: no row and no image leaves the device): (mtf [M, nf], otf [M, nf] complex, sums [M], stats [M, 12]) as PSFDetector.mtf gives
        them from host rows."""
        o = np.asarray(orientation, dtype=np.float64)
        e1, e2 = o[:, 0], o[:, 2]
        ptr, cnt, dev = self._psf_resident_rows(slot)
        rows = dict(device=dev, hits_device_ptr=ptr, n_hits=cnt)
        ms = []

        def timed(out):
            ms.append(out[-1])
            return out

        def window_fn():
            st, info = self.psf_stats(slot, position, o), self.psf_zernike(slot, position, o, order=0)[1]
            return st[abi.PSF_K_MAX], info[abi.ZERN_RHO], int(st[abi.PSF_N])

        out = cp.psf_mtf(lambda ax, off: timed(abi.psf_focus_stats(None, position, e1, e2, ax, off, **rows))[0],
                         lambda ax, off, fq, cen: timed(abi.psf_geo_otf(None, position, e1, e2, ax, off, fq, centers=cen, **rows))[:3],
                         lambda d, xs, zs, fq: timed(abi.psf_otf(None, position, e1, e2, d, xs, zs, fq, **rows))[:3],
                         window_fn, o, freqs, offsets=offsets, kind=kind, n=n, half_width=half_width, axis=axis, follow=follow)
        self.readout_ms = float(sum(ms))
        return out

    def psf_encircled_energy(self, slot, position, orientation, radii, offsets=(0.0,), kind="geometric", shape="circle", n=None, half_width=None, axis=None,
                             follow="centroid"):
        """The encircled or ensquared energy of the resident rows of PSFDetector slot `slot` (bmo_psf_focus_stats, then bmo_psf_geo_ee or
        bmo_psf_ee on the device pointer: no row and no image leaves the device): (ee [M, nr], energy [M, nr], sums [M], centers [M, 2],
        stats [M, 12]) as PSFDetector.encircled_energy gives them from host rows."""
        o = np.asarray(orientation, dtype=np.float64)
        e1, e2 = o[:, 0], o[:, 2]
        ptr, cnt, dev = self._psf_resident_rows(slot)
        rows = dict(device=dev, hits_device_ptr=ptr, n_hits=cnt)
        ms = []

        def timed(out):
            ms.append(out[-1])
            return out

        def window_fn():
            st, info = self.psf_stats(slot, position, o), self.psf_zernike(slot, position, o, order=0)[1]
            return st[abi.PSF_K_MAX], info[abi.ZERN_RHO], int(st[abi.PSF_N])

        def geo_fn(ax, off, r, cen, sh):
            ee, energy, _, sums, _ = timed(abi.psf_geo_ee(None, position, e1, e2, ax, off, r, centers=cen, shape=sh, want_count=False, **rows))
            return ee, energy, sums

        out = cp.psf_encircled_energy(lambda ax, off: timed(abi.psf_focus_stats(None, position, e1, e2, ax, off, **rows))[0], geo_fn,
                                      lambda d, xs, zs, r, sh: timed(abi.psf_ee(None, position, e1, e2, d, xs, zs, r, shape=sh, **rows))[:4],
                                      window_fn, o, radii, offsets=offsets, kind=kind, shape=shape, n=n, half_width=half_width, axis=axis, follow=follow)
        self.readout_ms = float(sum(ms))
        return out

    def psf_bands(self, slot, ks=None):
        """The resident rows of PSFDetector slot `slot` split by wave number on the device (bmo_psf_bands_create on the pointer of
        bmo_result_psf_rows: no row leaves the device): an abi.PsfBands, to be closed by the caller.  It owns a copy of the rows and outlives
        this solution."""
        ptr, cnt, dev = self._psf_resident_rows(slot)
        bands, self.readout_ms = abi.psf_bands(None, ks=ks, device=dev, hits_device_ptr=ptr, n_hits=cnt, want_ms=True)
        return bands

    def _psf_all_rows(self, slot):
        ptr, cnt, dev = self._psf_resident_rows(slot)
        return dict(hits=None, device=dev, hits_device_ptr=ptr, n_hits=cnt)

    def psf_chromatic_focus(self, slot, position, orientation, offsets, axis=None, ks=None, plane=None):
        """Where each colour of the resident rows of PSFDetector slot `slot` focuses and lands: (ks, stats [B, M, 12], focus [B], rms [B],
        centroids [B, 2], plane) as PSFDetector.chromatic_focus gives them from host rows."""
        with self.psf_bands(slot, ks=ks) as b:
            ms = self.readout_ms
            out, t = cp.chromatic_focus_of(b, position, orientation, offsets, axis=axis, plane=plane)
            self.readout_ms = ms + t
            return (b.ks.copy(),) + out

    def psf_poly_through_focus(self, slot, position, orientation, offsets, weights=None, n=100, normalize="energy", axis=None, follow="centroid",
                               window_plane=None, crop_factor=1.0, half_width=None, ks=None, want_bands=False):
        """The incoherent, spectrally weighted through-focus stack of the resident rows of PSFDetector slot `slot`: (xs, zs, displacements,
        I[M, n, n], stats, ks, coeffs, I_b or None) as PSFDetector.poly_through_focus gives them from host rows."""
        all_rows = self._psf_all_rows(slot)
        with self.psf_bands(slot, ks=ks) as b:
            ms = self.readout_ms
            out, t = cp.poly_through_focus_of(all_rows, b, position, orientation, offsets, weights=weights, n=n, normalize=normalize, axis=axis, follow=follow,
                                              window_plane=window_plane, crop_factor=crop_factor, half_width=half_width, want_bands=want_bands)
            self.readout_ms = ms + t
            return out[:5] + (b.ks.copy(),) + out[5:]

    def psf_poly_mtf(self, slot, position, orientation, freqs, offsets=(0.0,), weights=None, normalize="energy", n=None, half_width=None, axis=None,
                     follow="centroid", ks=None):
        """The white-light diffraction MTF of the resident rows of PSFDetector slot `slot`: (mtf [M, nf], otf [M, nf] complex, sums [M],
        stats [M, 12], ks, coeffs) as PSFDetector.poly_mtf gives them from host rows."""
        all_rows = self._psf_all_rows(slot)
        with self.psf_bands(slot, ks=ks) as b:
            ms = self.readout_ms
            out, t = cp.poly_mtf_of(all_rows, b, position, orientation, freqs, offsets=offsets, weights=weights, normalize=normalize, n=n,
                                    half_width=half_width, axis=axis, follow=follow)
            self.readout_ms = ms + t
            return out[:4] + (b.ks.copy(),) + out[4:]

    def spot_encircled_energy(self, slot, radii, center=None, shape="circle"):
        """bmo_spot_ee_sweep on the resident rows of Spotdetector slot `slot`: (fraction [nr], inside int64 [nr], n_rows) as
        Spotdetector.encircled_energy gives them from host rows; center None: the centroid of spot_stats(slot)."""
        ms = 0.0
        if center is None:
            center = cp.spot_ee_centers(self.spot_stats(slot))
            ms = self.readout_ms
        inside, n_rows, ms2 = abi.spot_ee_sweep(self.handle, slot, 1, center, radii, shape=shape)
        self.readout_ms = ms + ms2
        return cp.spot_ee_fraction(inside[0], int(n_rows[0])), inside[0], int(n_rows[0])

    def psf_intensity(self, slot, position, orientation, n=100, **window_kw):
        """intensity(psf; ...) of the resident rows of PSFDetector slot `slot`: (xs, zs, I[n, n]).  The window comes from psf_stats
        (components.psf_axes_from_stats takes window_kw), the image from bmo_psf_intensity_sweep: only the image leaves the device."""
        st = self.psf_stats(slot, position, orientation)
        ms = self.readout_ms
        if st[abi.PSF_N] == 0:
            raise ValueError("psf_intensity: the PSFDetector recorded no hit")
        xs, zs = cp.psf_axes_from_stats(st, n=n, **window_kw)
        o = np.asarray(orientation, dtype=np.float64)
        I, _, ms2 = abi.psf_intensity_sweep(self.handle, slot, 1, position, o[:, 0], o[:, 2], xs, zs)
        self.readout_ms = ms + ms2
        return xs, zs, I[0]


def _engine_solve(scene, bundle, r_max, prev, device=0, max_beams=0):
    """One solve on the HIP engine: bmo_trace, or bmo_retrace when `prev` (an EngineSolution) is given."""
    eng = Engine(scene, device, max_beams)
    try:
        batch, keep = make_batch(scene, bundle)
        h = C.c_void_p()
        o = eng.opts(r_max)
        if prev is None:
            abi.check(eng.lib, eng.lib.bmo_trace(eng.handle, C.byref(batch), C.byref(o), C.byref(h)), "bmo_trace")
        else:
            abi.check(eng.lib, eng.lib.bmo_retrace(eng.handle, C.byref(batch), prev.handle, C.byref(o), C.byref(h)), "bmo_retrace")
        sol = EngineSolution(eng.lib, h, bundle.n, bundle.kind)
        res = eng.result_view(h)
    finally:
        eng.close()
    return res, sol


def release(beams):
    """Free the solution kept for retracing (device memory of the segment log) of a solved beam / beam group."""
    roots = beams.beams if isinstance(beams, bm.BeamGroup) else (list(beams) if isinstance(beams, (list, tuple)) else [beams])
    for b in roots:
        sol = getattr(b, "_solution", None)
        if sol is not None:
            sol.free()
        b._solution = None


def _roots_of(beams):
    if isinstance(beams, bm.BeamGroup):
        return beams.beams
    if isinstance(beams, (list, tuple)):
        return list(beams)
    return [beams]


def _prepare(system, beams):
    """(roots, bundle of their first rays, compiled scene, solution of the previous solve of exactly these beams or None)."""
    roots = _roots_of(beams)
    bundle = bm.RayBundle.from_beams(roots)
    scene = CompiledScene(system, bundle.lambdas)
    prev = getattr(roots[0], "_solution", None) if roots else None
    if prev is not None:
        same = all(getattr(b, "_solution", None) is prev and getattr(b, "_sol_index", -1) == i for i, b in enumerate(roots))
        if not (same and prev.handle and prev.n_roots == len(roots) and prev.kind == bundle.kind):
            prev = None  # a different grouping than the one that was solved: treat as fresh beams
    return roots, bundle, scene, prev


def _apply(scene, res, sol, roots, hit_fix=None, defer=False):
    """Fill the beam objects from a TraceResult and append this solve's detector records (detectors are not reset, like the reference:
    Spotdetector.jl / PSFDetector.jl "Reset behavior").  `hit_fix(slot, hits)` may adjust the rows before they are appended.  With `defer`
    the Spot / PSF rows are not appended but left on the beam that made them (`_pending_hits`), for a caller that merges several solves into
    the reference's order (_trace_open_leaves)."""
    nodes = _fill_beams(scene, res, roots)
    for i, b in enumerate(roots):
        b._solution, b._sol_index = sol, i
    for slot, det in enumerate(scene.detectors):
        hits = res.detector_hits(slot)
        if hit_fix is not None:
            hits = hit_fix(slot, hits)
        if defer and det.kind != cp.O_PHOTODETECTOR:
            rows = hits[:, 0:2] if det.kind == cp.O_SPOT else hits
            for nd, row in zip(res.detector_nodes(slot), rows):
                nodes[int(nd)].__dict__.setdefault("_pending_hits", []).append((det, row))
            continue
        if det.kind == cp.O_SPOT:
            det.data = np.concatenate([det.data, hits[:, 0:2]], axis=0)
        elif det.kind == cp.O_PHOTODETECTOR:
            if len(hits):  # pd.field[i, j] += electric_field(gauss, r, z) * sqrt(proj) for every recorded beamlet (Photodetector.jl:85-105)
                sol.photodetector_field(slot, det.position(), det.orientation(), det.x, det.y, det.field)
        else:
            det.data = np.concatenate([det.data, hits], axis=0)
    return nodes


def _trace_open_leaves(system, roots, r_max, device):
    """solve_system!(...; retrace = false) on beams that were solved before (System.jl:449-458, solve_leaf! :470-475): nothing is re-walked;
    every beam of the trees whose LAST ray has no intersection is traced on from that ray (without a hint, up to r_max rays in the beam),
    everything else stays as it is.  The open last rays are traced as one fresh batch per distinct remaining length and spliced back.
    A batch applies ONE ray limit to all its beams, the remaining length of the beams it continues, while the reference gives every child
    born in the continuation the full r_max: children that ran into the batch's limit are open beams themselves and are continued by the next
    pass.  Detector rows are appended at the end, in the order the reference's loop makes them: root by root, breadth-first."""
    open_beams, queue = [], list(roots)
    while queue:  # BFS like solve_system!
        b = queue.pop(0)
        queue.extend(b.children)
        if b.rays[-1].intersection is None and len(b.rays) < r_max:
            open_beams.append(b)
    while open_beams:
        open_beams = _continue_open_beams(system, open_beams, r_max, device)
    for root in roots:  # solve_system!(bg) finishes root 1's whole tree before it starts root 2 (System.jl:463-468): one BFS per root
        queue = [root]
        while queue:
            b = queue.pop(0)
            queue.extend(b.children)
            for det, row in b.__dict__.pop("_pending_hits", []):
                det.data = np.concatenate([det.data, np.asarray(row)[None, :]], axis=0)
    for b in roots:  # the resident solution no longer describes these beams: the next solve traces them afresh
        sol = getattr(b, "_solution", None)
        if sol is not None:
            sol.free()
        b._solution = None
    return None


def _continue_open_beams(system, open_beams, r_max, device):
    """One pass of _trace_open_leaves; returns the beams born in it that ran into the pass's ray limit below r_max."""
    again = []
    by_left = {}
    for b in open_beams:
        by_left.setdefault(r_max - len(b.rays) + 1, []).append(b)
    for left, group in sorted(by_left.items()):
        gaussian = group[0].kind == bm.BEAM_GAUSSIAN
        heads = []
        for b in group:
            if gaussian:
                subs = []
                for part in (b.chief, b.waist, b.divergence):
                    sub = bm.Beam.__new__(bm.Beam)
                    sub.rays, sub.parent, sub.children, sub.status = [part.rays[-1]], None, [], 0
                    subs.append(sub)
                h = bm.GaussianBeamlet(None, None, _parts=(subs[0], subs[1], subs[2], b.lam, b.w0, b.E0))
                h.parent, h.children, h.status = None, [], 0
            else:
                h = bm.Beam.__new__(bm.Beam)
                h.rays, h.parent, h.children, h.status = [b.rays[-1]], None, [], 0
            heads.append(h)
        bundle = bm.RayBundle.from_beams(heads)
        if gaussian:
            # the lengths the beamlets have accumulated up to their open rays (bmo.h "31 planes"), folded exactly as a solve that had
            # never stopped would have folded them
            acc = np.zeros((6, len(group)))
            for i, b in enumerate(group):
                l0 = 0.0 if b.parent is None else b.parent.length()
                len_a, len_b = 0.0, l0
                opl_c = 0.0 if b.chief.parent is None else b.chief.parent.optical_path_length()
                for r in b.chief.rays[:-1]:
                    len_a += r.intersection.t
                    len_b += r.intersection.t
                    opl_c += r.intersection.t * r.n
                opl_w = opl_d = 0.0
                for r in b.waist.rays[:-1]:
                    opl_w += r.intersection.t * r.n
                for r in b.divergence.rays[:-1]:
                    opl_d += r.intersection.t * r.n
                acc[:, i] = (len_a, len_b, l0, opl_c, opl_w, opl_d)
            bundle = bm.RayBundle(bundle.kind, np.vstack([bundle.planes, acc]))
        scene = CompiledScene(system, bundle.lambdas)
        res, sol = _engine_solve(scene, bundle, left, None, device)
        if gaussian and any(isinstance(o, cp.Photodetector) for o in system.objects()):
            # the field of a beamlet on a Photodetector is a function of ALL its rays (point_on_beam, length, optical_path_length:
            # Beam.jl:125-205); the continuation holds only those from the open ray on, the ones in front of it go along as a prefix
            starts, cols, opl_par = [0], [], []
            for b in group:
                for k in range(len(b.chief.rays) - 1):
                    col = []
                    for part in (b.chief, b.waist, b.divergence):
                        r = part.rays[k]
                        col += [r.pos[0], r.pos[1], r.pos[2], r.dir[0], r.dir[1], r.dir[2], r.n, r.intersection.t]
                    cols.append(col)
                starts.append(len(cols))
                opl_par.append(0.0 if b.chief.parent is None else b.chief.parent.optical_path_length())
            segs = np.asarray(cols, dtype=np.float64).T if cols else np.zeros((24, 0))
            sol.set_gauss_prefix(starts, segs, opl_par)
        # optical path length of each beam (parents included) up to the start of its open ray: what PSF records of the continuation add
        opl0 = []
        for b in group:
            acc = 0.0 if b.parent is None else b.parent.optical_path_length()
            for r in b.rays[:-1]:
                acc += r.optical_path_length()
            opl0.append(acc)

        def hit_fix(slot, hits, res=res, scene=scene, opl0=opl0, gaussian=gaussian):
            if gaussian or scene.detectors[slot].kind != cp.O_PSF or not len(hits):  # (a continued beamlet brings its path lengths along)
                return hits
            hits = hits.copy()
            root_of_hit = res.node_root[res.detector_nodes(slot)]
            hits[:, 6] += np.asarray(opl0)[root_of_hit]
            return hits

        nodes = _apply(scene, res, sol, heads, hit_fix, defer=True)
        sol.free()
        for b, h in zip(group, heads):
            if gaussian:
                for part, hp in ((b.chief, h.chief), (b.waist, h.waist), (b.divergence, h.divergence)):
                    part.rays[-1:] = hp.rays
                for c in h.children:
                    c.chief.parent = b.chief  # parent! Gaussian.jl:113-117
            else:
                b.rays[-1:] = h.rays  # the open ray (now with its intersection, if any) and what followed it
            b.status = h.status
            for c in h.children:
                c.parent = b
            b.children = h.children
            pend = h.__dict__.pop("_pending_hits", None)
            if pend:
                b.__dict__.setdefault("_pending_hits", []).extend(pend)
        if left < r_max:
            again += [nd for nd in nodes[len(group):] if (nd.status & abi.NODE_RMAX) and nd.rays[-1].intersection is None and len(nd.rays) < r_max]
    return again


def solve_system(system, beams, r_max=100, retrace=True, device=0):
    """solve_system!(system, beam | beam group; r_max=100, retrace=true) — src/System.jl:444-468.

    Fresh beams are traced; beams solved by an earlier call are RETRACED (System.jl:188-255, :326-428): the stored path is
    re-walked against the system as it is now, the first ray of every root supplying the (possibly modified) head.
    With retrace=False solved beams are not re-walked: only leaves whose last ray has no intersection are traced on (System.jl:470-475).
    Mutates the beam objects (rays, intersections, children) and appends detector data, exactly like the reference
    (detectors are not reset, Spotdetector.jl / PSFDetector.jl "Reset behavior").  Returns the raw TraceResult (None for retrace=False
    on solved beams).  The backend is the HIP engine, always: there is no other.
    """
    roots, bundle, scene, prev = _prepare(system, beams)
    if prev is not None and not retrace:
        return _trace_open_leaves(system, roots, r_max, device)
    res, sol = _engine_solve(scene, bundle, r_max, prev, device)
    _apply(scene, res, sol, roots)
    return res


# ---------------------------------------------------------------------------------------- sweeps
def _fresh_head(b):
    """A fresh (un-solved) copy of the head of root beam `b`, of the kind _fill_beams fills: its own rays come from the result."""
    if b.kind == bm.BEAM_GAUSSIAN:
        subs = []
        for part in (b.chief, b.waist, b.divergence):
            sub = bm.Beam.__new__(bm.Beam)
            sub.rays, sub.parent, sub.children, sub.status = [part.rays[0]], None, [], 0
            subs.append(sub)
        h = bm.GaussianBeamlet(None, None, _parts=(subs[0], subs[1], subs[2], b.lam, b.w0, b.E0))
    else:
        h = bm.Beam.__new__(bm.Beam)
        h.rays = [b.rays[0]]
    h.parent, h.children, h.status = None, [], 0
    return h


def _first_rec(res, i):
    """First segment of node i of a TraceResult in the whole log's numbering (i = n_nodes: one past the last)."""
    if i < res.n_nodes:
        return int(res.node_first_rec[i])
    return int(res.node_first_rec[-1]) + int(res.node_nseg[-1]) if res.n_nodes else 0


class _ResultSlice:
    """The nodes, records and statuses of one configuration of a sweep's TraceResult, renumbered as a solve of that configuration alone."""

    def __init__(self, res, n0, n1, r0, r1, root0):
        # (a detector-only solve, record_segments = 0, keeps the segment numbering of the beams but no records)
        self.beam_kind, self.n_nodes, self.n_records = res.beam_kind, n1 - n0, (r1 - r0) if res.n_records else 0
        self.node_root = res.node_root[n0:n1] - root0
        par = res.node_parent[n0:n1]
        self.node_parent = np.where(par >= 0, par - n0, -1).astype(np.int32)
        fc = res.node_first_child[n0:n1]
        self.node_first_child = np.where(fc >= 0, fc - n0, -1).astype(np.int32)
        self.node_first_rec = res.node_first_rec[n0:n1] - r0
        self.node_nseg = res.node_nseg[n0:n1]
        self.node_status = res.node_status[n0:n1]
        self.node_aux = res.node_aux[n0:n1]
        self.rec = res.rec[:, r0:r1]
        self.rec_obj = res.rec_obj[r0:r1]
        self.rec_shape = res.rec_shape[r0:r1]


class SweepSolution:
    """The solution of n configurations of one system (bmo.solve_sweep): configuration c is a fresh solve_system of snapshot c."""

    def __init__(self, lib, handle, res, scenes, heads, poses, grids):
        self.lib, self._handle, self.res = lib, handle, res
        self.scenes, self._heads, self._poses, self._grids = scenes, heads, poses, grids
        self.n = len(scenes)
        self.n_roots = len(heads)  # roots per configuration
        nr = self.n_roots
        # node range of every configuration: nodes are in root order, the roots of configuration c are c * nr .. (c + 1) * nr - 1
        self._node_start = np.searchsorted(res.node_root, np.arange(self.n + 1) * nr).astype(np.int64)
        ns = self._node_start
        self._rec_start = np.array([_first_rec(res, i) for i in ns], dtype=np.int64)

    def close(self):
        if self._handle:
            self.lib.bmo_result_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _slot(self, det):
        for slot, d in enumerate(self.scenes[0].detectors):
            if d is det:
                return slot
        raise KeyError("detector is not part of the swept system")

    def result(self, c):
        """The nodes, records and statuses of configuration c (the layout of abi.TraceResult, numbered from 0)."""
        n0, n1 = int(self._node_start[c]), int(self._node_start[c + 1])
        return _ResultSlice(self.res, n0, n1, int(self._rec_start[c]), int(self._rec_start[c + 1]), c * self.n_roots)

    def beams(self, c):
        """Beam / GaussianBeamlet trees of configuration c, as solve_system would leave fresh copies of the root beams."""
        roots = [_fresh_head(b) for b in self._heads]
        sl = self.result(c)
        _fill_beams(self.scenes[c], sl, roots)
        return roots

    def _hit_rows(self, slot, c):
        nodes = self.res.detector_nodes(slot)
        cfg = self.res.node_root[nodes] // max(1, self.n_roots)
        return self.res.detector_hits(slot)[cfg == c]

    def spot_hits(self, det, c):
        """Rows a Spotdetector records in configuration c (x, y per hit, Spotdetector.jl:59), in the reference's order."""
        return self._hit_rows(self._slot(det), c)[:, 0:2]

    def detector_hits(self, det, c):
        """All nine columns of the hit rows of detector `det` in configuration c (include/bmo.h det_data)."""
        return self._hit_rows(self._slot(det), c)

    def photodetector_field(self, pd):
        """Complex field [n, nx, ny] of Photodetector `pd` in every configuration (one batched read-out, bmo_photodetector_field_sweep)."""
        slot = self._slot(pd)
        xs, ys = self._grids[slot]
        nx, ny, K = len(xs), len(ys), self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([np.asarray(self._poses[c][slot][1]).reshape(9) for c in range(K)], dtype=np.float64)
        buf = np.zeros(2 * K * nx * ny)
        dp = C.POINTER(C.c_double)
        ms = C.c_double()
        x, y = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
        abi.check(self.lib, self.lib.bmo_photodetector_field_sweep(self._handle, int(slot), int(K), pos.ctypes.data_as(dp), ori.ctypes.data_as(dp),
                                                                   x.ctypes.data_as(dp), y.ctypes.data_as(dp), nx, ny, buf.ctypes.data_as(dp), C.byref(ms)),
                  "bmo_photodetector_field_sweep")
        self.readout_ms = ms.value
        f = (buf[0::2] + 1j * buf[1::2]).reshape(K, ny, nx)  # (i, j) at [i + nx*j]
        return np.ascontiguousarray(f.transpose(0, 2, 1))

    def psf_intensity(self, det, n=100, crop_factor=1, center="centroid", x_min=math.inf, x_max=math.inf, z_min=math.inf, z_max=math.inf,
                      x0_shift=0, z0_shift=0, axes=None, want_field=False, window="host"):
        """intensity(psf; ...) of PSFDetector `det` in every configuration, in one batched read-out (bmo_psf_intensity_sweep): (xs[n_cfg, n],
        zs[n_cfg, n], I[n_cfg, n, n]), and the complex field [n_cfg, n, n] as well with `want_field`.  Configuration c samples the axes
        PSFDetector.sample_axes gives for its rows at its detector pose, and equals PSFDetector.intensity after a solve of its snapshot bit for
        bit.  axes=(xs, zs) samples every configuration on that one window instead (a through-focus comparison); without it a configuration
        whose detector recorded no hit has no window, a ValueError.  window="device" takes every configuration's axes from one psf_stats
        read-out (components.psf_axes_from_stats) instead of the host copy of the rows: the same rule, with the centroid summed in the
        device's order, so the axes may differ from the "host" ones in their last bits."""
        if window not in ("host", "device"):
            raise ValueError('psf_intensity: window must be "host" or "device"')
        slot = self._slot(det)
        K = self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([self._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        if axes is not None:
            ax, az = (np.asarray(a, dtype=np.float64) for a in axes)
            if ax.ndim != 1 or ax.shape != az.shape:
                raise ValueError("psf_intensity: axes must be two 1-D arrays of one length")
            xs, zs = np.tile(ax, (K, 1)), np.tile(az, (K, 1))
            stats_ms = 0.0
        elif window == "device":
            st, stats_ms = abi.psf_stats_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2])
            empty = np.flatnonzero(st[:, abi.PSF_N] == 0)
            if len(empty):
                raise ValueError(f"psf_intensity: the PSFDetector recorded no hit in configuration {empty[0]}; pass axes=(xs, zs) to read it")
            xs, zs = cp.psf_axes_from_stats(st, n=n, crop_factor=crop_factor, center=center, x_min=x_min, x_max=x_max, z_min=z_min, z_max=z_max,
                                            x0_shift=x0_shift, z0_shift=z0_shift)
        else:
            stats_ms = 0.0
            nodes = self.res.detector_nodes(slot)
            cfg = self.res.node_root[nodes] // max(1, self.n_roots)
            start = np.searchsorted(cfg, np.arange(K + 1))  # rows are in configuration order
            rows = self.res.detector_hits(slot)
            xs, zs = np.zeros((K, int(n))), np.zeros((K, int(n)))
            for c in range(K):
                if start[c] == start[c + 1]:
                    raise ValueError(f"psf_intensity: the PSFDetector recorded no hit in configuration {c}; pass axes=(xs, zs) to read it")
                xs[c], zs[c] = cp.psf_sample_axes(rows[start[c]:start[c + 1]], pos[c], ori[c], n=n, crop_factor=crop_factor, center=center,
                                                  x_min=x_min, x_max=x_max, z_min=z_min, z_max=z_max, x0_shift=x0_shift, z0_shift=z0_shift)
        I, field, ms = abi.psf_intensity_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], xs, zs, want_field=want_field)
        self.readout_ms = ms + stats_ms
        return (xs, zs, I, field) if want_field else (xs, zs, I)

    def psf_stats(self, det, ref=None):
        """The wavefront statistics [n_cfg, 21] (abi.PSF_* columns) of PSFDetector `det` in every configuration, in one batched read-out
        (bmo_psf_stats_sweep) at each configuration's detector pose; ref: None (each centroid), one (x, z) or [n_cfg, 2].  Row c equals
        abi.psf_stats on detector_hits(det, c) bit for bit, a configuration without rows reads N = 0 and NaN."""
        slot = self._slot(det)
        K = self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([self._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        st, self.readout_ms = abi.psf_stats_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], ref=ref)
        return st

    def psf_zernike(self, det, order=4, ref=None, pupil=None, want_gram=False):
        """The Zernike fit of the wavefront of PSFDetector `det` in every configuration, in one batched read-out (bmo_psf_zernike_sweep) at
        each configuration's detector pose: (coef [n_cfg, J], info [n_cfg, 13] at the abi.ZERN_* columns), with want_gram also the packed
        normal equations [n_cfg, E].  ref: None, one (x, z) or [n_cfg, 2]; pupil: None, one (U0, V0, RHO) or [n_cfg, 3].  Row c equals
        abi.psf_zernike on detector_hits(det, c) bit for bit; a configuration without rows reads N = 0, STATUS = 1 and NaN."""
        slot = self._slot(det)
        K = self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([self._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        coef, info, gram, self.readout_ms = abi.psf_zernike_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], order=order, ref=ref, pupil=pupil,
                                                                  want_gram=want_gram)
        return (coef, info, gram) if want_gram else (coef, info)

    def psf_opd_map(self, det, n=64, order=4, remove="tilt", ref=None, pupil=None, coef=None):
        """The binned wavefront (OPD) map of PSFDetector `det` in every configuration, in one batched read-out (bmo_psf_opd_map_sweep, after
        one bmo_psf_zernike_sweep where `remove` asks for a fit) at each configuration's detector pose: (opd [n_cfg, n, n] indexed
        [c, i, j], weight, count, info [n_cfg, 20] at the abi.OPD_* columns, coef_removed [n_cfg, J]) as components.psf_opd_map describes
        them.  ref, pupil and coef (a surface to remove as it stands, instead of `remove`): None, one value or one per configuration.
        Configuration c equals abi.psf_opd_map on detector_hits(det, c) bit for bit."""
        slot = self._slot(det)
        K = self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([self._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        ms = []

        def zernike_fn(od, r, q):
            cf, info, _, t = abi.psf_zernike_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], order=od, ref=r, pupil=q)
            ms.append(t)
            return cf, info

        def map_fn(od, cf, r, q):
            out = abi.psf_opd_map_sweep(self._handle, slot, K, pos, ori[:, :, 0], ori[:, :, 2], n=n, order=od, coef=cf, ref=r, pupil=q)
            ms.append(out[5])
            return out[:4]

        if coef is not None:
            coef = abi._per_config(coef, K, abi.zernike_sizes(order)[0])
        out = cp.psf_opd_map(zernike_fn, map_fn, n=n, order=order, remove=remove, ref=ref, pupil=pupil, coef=coef)
        self.readout_ms = float(sum(ms))
        return out

    def _focus_planes(self, det, offsets, axis, follow, who):
        """(slot, pos [K, 3], ori [K, 3, 3], axes [K, 3], offsets [K, M]) of a through-focus read-out of every configuration: `offsets` one
        list for all or [K, M], `axis` None (each configuration's local y), one vector for all or [K, 3]."""
        slot = self._slot(det)
        K = self.n
        pos = np.ascontiguousarray([self._poses[c][slot][0] for c in range(K)], dtype=np.float64)
        ori = np.ascontiguousarray([self._poses[c][slot][1] for c in range(K)], dtype=np.float64)
        off = abi._sweep_planes(K, offsets)
        ax = None if axis is None else abi._per_config(axis, K, 3)
        planes = [cp.focus_planes(ori[c], off[c], None if ax is None else ax[c], follow, who) for c in range(K)]
        return slot, pos, ori, np.ascontiguousarray([p[0] for p in planes]), np.ascontiguousarray([p[1] for p in planes])

    def psf_focus_stats(self, det, offsets, axis=None):
        """The focus statistics [n_cfg, M, 12] (abi.FOCUS_* columns) of PSFDetector `det` in every configuration, in one batched read-out
        (bmo_psf_focus_stats_sweep): the rows of configuration c propagated to its detector plane moved by offsets[m] (one list for all
        configurations, or [n_cfg, M]) along `axis` (None: its local y).  Block c equals abi.psf_focus_stats on detector_hits(det, c) bit for
        bit; a configuration without rows reads N = 0 and NaN."""
        slot, pos, ori, ax, off = self._focus_planes(det, offsets, axis, "centroid", "psf_focus_stats")
        st, self.readout_ms = abi.psf_focus_stats_sweep(self._handle, slot, self.n, pos, ori[:, :, 0], ori[:, :, 2], ax, off)
        return st

    def psf_best_focus(self, det, offsets, column=abi.FOCUS_RMS_R, kind="min"):
        """(offset [n_cfg], value [n_cfg]) of the extremum of the focus curve of every configuration: components.best_focus on column
        `column` of psf_focus_stats(det, offsets); NaN for a configuration without statistics."""
        st = self.psf_focus_stats(det, offsets)
        off = abi._sweep_planes(self.n, offsets)
        best = np.full((self.n, 2), np.nan)
        for c in range(self.n):
            if not np.isnan(st[c, :, column]).all():
                best[c] = cp.best_focus(off[c], st[c, :, column], kind=kind)
        return best[:, 0].copy(), best[:, 1].copy()

    def _through_focus_plans(self, st, ori, ax, off, n, plan_kw):
        """components.through_focus_plan for every configuration with rows, from the focus statistics st [K, M, 12]: (xs [K, n], zs [K, n],
        displacements [K, M, 3]), NaN for a configuration without rows (its stack reads zeros whatever they hold)."""
        K, M = off.shape
        xs, zs, d = np.full((K, int(n)), np.nan), np.full((K, int(n)), np.nan), np.full((K, M, 3), np.nan)
        for c in range(K):
            if st[c, 0, abi.FOCUS_N] > 0:
                kw = {k: (v[c] if k == "half_width" and v is not None and np.ndim(v) == 2 else v) for k, v in plan_kw.items()}
                try:
                    xs[c], zs[c], d[c] = cp.through_focus_plan(st[c], ori[c], ax[c], off[c], n=n, **kw)
                except ValueError as e:
                    raise ValueError("configuration %d: %s" % (c, e)) from None
        return xs, zs, d

    def psf_through_focus(self, det, offsets, n=100, axis=None, follow="centroid", window_plane=None, crop_factor=1.0, half_width=None):
        """The through-focus PSF stack of PSFDetector `det` in every configuration, in two batched read-outs (bmo_psf_focus_stats_sweep, then
        bmo_psf_through_focus_sweep: no row leaves the device): (xs [n_cfg, n], zs [n_cfg, n], displacements [n_cfg, M, 3],
        I[n_cfg, M, n, n], stats [n_cfg, M, 12]).  Block c is what components.psf_through_focus gives on detector_hits(det, c) at
        configuration c's pose, bit for bit.  half_width: None, one number, (hwx, hwz), or [n_cfg, 2].  A configuration without rows does not
        raise: its axes and displacements are NaN, its images 0, its statistics N = 0 and NaN."""
        slot, pos, ori, ax, off = self._focus_planes(det, offsets, axis, follow, "through_focus")
        st, ms0 = abi.psf_focus_stats_sweep(self._handle, slot, self.n, pos, ori[:, :, 0], ori[:, :, 2], ax, off)
        xs, zs, d = self._through_focus_plans(st, ori, ax, off, n, dict(follow=follow, window_plane=window_plane, crop_factor=crop_factor, half_width=half_width))
        I, _, ms1 = abi.psf_through_focus_sweep(self._handle, slot, self.n, pos, ori[:, :, 0], ori[:, :, 2], d, xs, zs)
        self.readout_ms = ms0 + ms1
        return xs, zs, d, I, st

    def psf_mtf(self, det, freqs, offsets=(0.0,), kind="diffraction", n=None, half_width=None, axis=None, follow="centroid"):
        """The MTF of PSFDetector `det` in every configuration at `freqs` [nf, 2] (cycles per metre, shared by all), in batched read-outs
        (bmo_psf_focus_stats_sweep, then bmo_psf_geo_otf_sweep or bmo_psf_otf_sweep: no row and no image leaves the device):
        (mtf [n_cfg, M, nf], otf [n_cfg, M, nf] complex, sums [n_cfg, M], stats [n_cfg, M, 12]) as components.psf_mtf describes them.
        kind "diffraction": half_width None takes components.mtf_window's for every configuration (from one psf_stats_sweep and one
        psf_zernike_sweep of order 0), n None the largest n any configuration's window asks for; block c equals components.psf_mtf on
        detector_hits(det, c) given that n and configuration c's half-width, bit for bit.  A configuration without rows does not raise: its
        mtf is NaN, its otf and sums 0."""
        if kind not in ("diffraction", "geometric"):
            raise ValueError('mtf: kind must be "diffraction" or "geometric"')
        fq = np.asarray(freqs, dtype=np.float64).reshape(-1, 2)
        if len(fq) == 0 or not np.isfinite(fq).all():
            raise ValueError("mtf: needs at least one frequency, all finite")
        slot, pos, ori, ax, off = self._focus_planes(det, offsets, axis, follow, "mtf")
        K = self.n
        e1s, e2s = ori[:, :, 0], ori[:, :, 2]
        st, ms = abi.psf_focus_stats_sweep(self._handle, slot, K, pos, e1s, e2s, ax, off)
        full = [c for c in range(K) if st[c, 0, abi.FOCUS_N] > 0]
        if kind == "geometric":
            centers = np.full((K, off.shape[1], 2), np.nan)
            for c in full:
                centers[c] = cp.mtf_geo_centers(st[c], follow)
            mtf, otf, sums, ms1 = abi.psf_geo_otf_sweep(self._handle, slot, K, pos, e1s, e2s, ax, off, fq, centers=centers)
            self.readout_ms = ms + ms1
            return mtf, otf, sums, st
        hw = None if half_width is None else np.broadcast_to(np.asarray(half_width, dtype=np.float64), (K, 2)).copy()
        if hw is None:
            wst, ms1 = abi.psf_stats_sweep(self._handle, slot, K, pos, e1s, e2s)
            _, info, _, ms2 = abi.psf_zernike_sweep(self._handle, slot, K, pos, e1s, e2s, order=0)
            ms += ms1 + ms2
            hw, n_rule = np.full((K, 2), np.nan), 2
            for c in full:
                try:
                    hw[c], n_c = cp.mtf_image_grid((wst[c, abi.PSF_K_MAX], info[c, abi.ZERN_RHO], int(wst[c, abi.PSF_N])), fq)
                except ValueError as e:
                    raise ValueError("configuration %d: %s" % (c, e)) from None
                n_rule = max(n_rule, n_c)
        else:
            n_rule = max([2] + [cp.mtf_image_grid(None, fq, half_width=hw[c])[1] for c in full])
        n = n_rule if n is None else int(n)
        xs, zs, d = self._through_focus_plans(st, ori, ax, off, n, dict(follow=follow, half_width=hw))
        for c in full:
            cp.mtf_check_pitch(xs[c], zs[c], fq)
        mtf, otf, sums, _, ms3 = abi.psf_otf_sweep(self._handle, slot, K, pos, e1s, e2s, d, xs, zs, fq)
        self.readout_ms = ms + ms3
        return mtf, otf, sums, st

    def spot_stats(self, det):
        """The spot statistics [n_cfg, 12] (abi.SPOT_* columns) of Spotdetector `det` in every configuration, in one batched read-out
        (bmo_spot_stats_sweep); row c equals abi.spot_stats on spot_hits(det, c) bit for bit, a configuration without rows reads N = 0 and NaN."""
        st, self.readout_ms = abi.spot_stats_sweep(self._handle, self._slot(det), self.n)
        return st

    def spot_image(self, det, nx, nz=None, window=None):
        """The spot diagram of Spotdetector `det` in every configuration as images, in one batched read-out (bmo_spot_image_sweep):
        (windows [n_cfg, 4], counts int64 [n_cfg, nx, nz] indexed [c, i, j], outside [n_cfg]).  window: one (x0, x1, z0, z1) for all
        configurations, None for the detector face, an array [n_cfg, 4], or "extent" for the extrema of each configuration's rows (ValueError
        naming the first configuration without rows or with a zero extent).  Binning is the floor rule of Spotdetector.image."""
        slot = self._slot(det)
        K = self.n
        if window is None:
            window = (-det.hw, det.hw, -det.hw, det.hw)
        if isinstance(window, str):
            if window != "extent":
                raise ValueError('spot_image: window must be (x0, x1, z0, z1), [n_cfg, 4], None or "extent"')
            st = self.spot_stats(det)
            w = np.array([cp.spot_extent_window(st[c], f"spot_image: configuration {c}") for c in range(K)], dtype=np.float64)
        else:
            w = np.asarray(window, dtype=np.float64)
            w = np.tile(w, (K, 1)) if w.ndim == 1 else w.reshape(K, 4)
        img, outside, self.readout_ms = abi.spot_image_sweep(self._handle, slot, K, w, nx, nz)
        return w, img, outside

    def spot_encircled_energy(self, det, radii, center=None, shape="circle"):
        """The share of the rows of Spotdetector `det` inside a circle or a square of every half-size of `radii`, in every configuration, in
        one batched read-out (bmo_spot_ee_sweep): (fraction [n_cfg, nr], inside int64 [n_cfg, nr], n_rows int64 [n_cfg], centers [n_cfg, 2]).
        center: one (x, z) for all configurations, an array [n_cfg, 2], or None for each configuration's centroid (one spot_stats call).
        Row c equals abi.spot_ee on spot_hits(det, c) about its centre; a configuration without rows reads 0 and a NaN fraction."""
        slot = self._slot(det)
        K = self.n
        ms = 0.0
        if center is None:
            c = cp.spot_ee_centers(self.spot_stats(det))
            ms = self.readout_ms
        else:
            c = np.asarray(center, dtype=np.float64)
            c = np.tile(c, (K, 1)) if c.ndim == 1 else c.reshape(K, 2)
        inside, n_rows, ms2 = abi.spot_ee_sweep(self._handle, slot, K, c, radii, shape=shape)
        self.readout_ms = ms + ms2
        return cp.spot_ee_fraction(inside, n_rows), inside, n_rows, c

    def optical_power(self, pd, field=None):
        """optical_power(pd) of every configuration, [n]: the trapezoid rule of Photodetector.optical_power on each configuration's field."""
        slot = self._slot(pd)
        xs, ys = self._grids[slot]
        f = self.photodetector_field(pd) if field is None else field
        I = (f.real ** 2 + f.imag ** 2) / (2 * la.Z_vacuum)
        inner = np.sum((I[:, 1:, :] + I[:, :-1, :]) * np.diff(xs)[None, :, None], axis=1) / 2
        return np.sum((inner[:, 1:] + inner[:, :-1]) * np.diff(ys)[None, :], axis=1) / 2


def sweep_snapshots(system, lambdas, n, configure):
    """configure(c), then a CompiledScene snapshot of `system`, for c = 0 .. n - 1 in order: (scenes, detector poses per scene, detector
    grids).  A snapshot holds copies of the numbers, so later configure calls do not change it.  A Photodetector's grid must not change."""
    scenes, poses, grids = [], [], None
    for c in range(n):
        configure(c)
        sc = CompiledScene(system, lambdas)
        scenes.append(sc)
        poses.append([(np.array(d.position(), dtype=np.float64), np.array(d.orientation(), dtype=np.float64)) for d in sc.detectors])
        g = [(np.array(getattr(d, "x", ())), np.array(getattr(d, "y", ()))) for d in sc.detectors]
        if grids is None:
            grids = g
        else:
            for d, (x0, y0), (x1, y1) in zip(sc.detectors, grids, g):
                if d.kind == cp.O_PHOTODETECTOR and not (np.array_equal(x0, x1) and np.array_equal(y0, y1)):
                    raise ValueError(f"solve_sweep: the resolution of a Photodetector changed in configuration {c}")
    return scenes, poses, grids


def sweep_trace(scenes, bundle, root_config, r_max=100, device=0, record_segments=True, view=True):
    """bmo_scene_create_sweep over the snapshots `scenes` + bmo_trace_sweep of `bundle`, root i in configuration root_config[i]
    (non-decreasing).  Returns (abi.TraceResult or None without `view`, result handle, library); the caller frees the handle."""
    lib = abi.load_engine()
    n = len(scenes)
    descs = (abi.SceneDesc * n)(*[s.desc for s in scenes])
    handle = C.c_void_p()
    abi.check(lib, lib.bmo_scene_create_sweep(descs, n, C.byref(handle)), "bmo_scene_create_sweep")
    try:
        batch, keep = make_batch(scenes[0], bundle)
        cfg = np.ascontiguousarray(root_config, dtype=np.int32)
        o = abi.TraceOpts()
        o.r_max, o.device, o.record_segments, o.max_beams = int(r_max), int(device), int(bool(record_segments)), 0
        h = C.c_void_p()
        abi.check(lib, lib.bmo_trace_sweep(handle, C.byref(batch), cfg.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(o), C.byref(h)), "bmo_trace_sweep")
    finally:
        lib.bmo_scene_destroy(handle)
    if not view:
        return None, h, lib
    try:
        v = abi.ResultView()
        abi.check(lib, lib.bmo_result_view(h, C.byref(v)), "bmo_result_view")
        return abi.TraceResult(v), h, lib
    except Exception:
        lib.bmo_result_free(h)
        raise


def solve_sweep(system, beams, n, configure, r_max=100, device=0, record_segments=True):
    """Solve n configurations of `system` in one trace.  configure(c) is called for c = 0 .. n - 1 in order and sets the system up for
    configuration c (moves, parameter changes; the topology must stay: include/bmo.h "Sweeps"); a snapshot is compiled after each call.
    Every configuration traces fresh copies of the root beams (their heads are read; `beams` is not mutated) and equals, bit for bit, a
    fresh solve_system of its snapshot.  Detectors are not filled: read them from the returned SweepSolution.  The system is left as
    configure(n - 1) made it."""
    n = int(n)
    if n < 1:
        raise ValueError("solve_sweep: n must be at least 1")
    heads = _roots_of(beams)
    if not heads:
        raise ValueError("solve_sweep: no beams")
    bundle = bm.RayBundle.from_beams(heads)
    scenes, poses, grids = sweep_snapshots(system, bundle.lambdas, n, configure)
    nr = bundle.n
    res, h, lib = sweep_trace(scenes, bm.RayBundle(bundle.kind, np.tile(bundle.planes, (1, n))), np.repeat(np.arange(n, dtype=np.int32), nr),
                              r_max, device, record_segments)
    return SweepSolution(lib, h, res, scenes, heads, poses, grids)
