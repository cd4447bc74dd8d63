/*
 * bmo.h — C ABI of the MI355X-native trace engine for BeamletOptics.jl's hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI; the
 * entry points below replace, for a whole batch of beams at once,
 *
 *   solve_system!(system, bg::AbstractBeamGroup; r_max, retrace)   src/System.jl:463-468
 *   solve_system!(system, beam::AbstractBeam;   r_max, retrace)    src/System.jl:444-461
 *     -> trace_system!(system, beam::Beam)                          src/System.jl:130-154
 *     -> trace_system!(system, gauss::GaussianBeamlet)              src/System.jl:274-318
 *     -> tracing_step! / trace_one / trace_all                      src/System.jl:57-110
 *     -> intersect3d(object|shape, ray)                             src/AbstractTypes/AbstractRay.jl:118-155,
 *                                                                   src/Mesh.jl:244-267, src/SDFs/AbstractSDF.jl:166-181
 *     -> interact3d(system, object, beam, ray)                      src/OpticalComponents/ (all files)
 *
 * Everything is plain C: pointers + sizes, FP64, SI metres.  No exceptions cross
 * the boundary: functions return 0 on success or a negative bmo_status code and
 * bmo_last_error() gives the thread-local message.  Data-dependent faults that
 * are exceptions in the reference (non-unit vectors OpticUtils.jl:33-35, ...)
 * are reported per beam node in node_status so the wrapper can re-raise them.
 *
 * Threading: a bmo_scene is immutable after creation and may be shared between threads; trace / retrace calls may be issued
 * from several host threads (the reference's trace loop is single-threaded, System.jl:239, :403) — calls for the same device
 * are serialised inside the library (one trace stream per device), calls for different devices run concurrently.  A
 * bmo_trace_result may be read (view, hits, retrace source, read-outs) from one thread at a time.
 *
 * The library is libbmo_hip.so (HIP, gfx950).  There is no CPU fallback inside
 * it: every trace call needs a GPU and fails with BMO_ERR_NO_DEVICE otherwise.
 * The independent CPU restatement of the reference algorithm lives in oracle/
 * (test infrastructure) and exports bmo_cpu_trace() with the same descriptor.
 */
#ifndef BMO_H
#define BMO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BMO_ABI_VERSION 1

/* ------------------------------------------------------------------ status */
enum bmo_status {
    BMO_OK = 0,
    BMO_ERR_INVALID = -1,     /* bad descriptor / argument                     */
    BMO_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure           */
    BMO_ERR_OOM = -3,         /* device or host allocation failed              */
    BMO_ERR_UNSUPPORTED = -4, /* shape/object/beam kind not built yet          */
    BMO_ERR_INTERNAL = -5,
    BMO_ERR_LIMIT = -6        /* bmo_trace_opts.max_beams exceeded             */
};

/* per-node status bits (node_status) */
enum bmo_node_status {
    BMO_NODE_MISS = 1,        /* last segment found no intersection (System.jl:142-144)   */
    BMO_NODE_STOPPED = 2,     /* interact3d returned nothing (System.jl:147-149)          */
    BMO_NODE_RMAX = 4,        /* length(rays) reached r_max (System.jl:133)               */
    BMO_NODE_SPLIT = 8,       /* children!(beam,[t,r]) was called (ThinBeamsplitter.jl:108-115) */
    BMO_NODE_DETECTED = 16,   /* a detector recorded this beam                            */
    BMO_NODE_ERR_UNIT = 32,   /* refraction3d unit-length ArgumentError (OpticUtils.jl:33-35) */
    BMO_NODE_GAUSS_DIVERGED = 64, /* chief/waist/div did not hit same shape (System.jl:298-304) */
    BMO_NODE_BLOCKED = 128,   /* PolarizationFilter blocked ray (PolarizationFilter.jl:42) */
    BMO_NODE_ERR_ORTHO = 256, /* E0 not orthogonal to dir, ErrorException (PolarizedRays.jl:54-56) */
    BMO_NODE_RETRACE_STALE = 512 /* retrace only, a NOTE (the result is the reference's): retrace_system! acted on stale data here.
                                    (i) The stored beam had children and the re-walk ended in a `nothing` interaction before
                                    reaching the splitter: the reference sets no cleanup flag (System.jl:232-239), keeps the
                                    children and retraces each from its stored first ray — so does this library (the beam then
                                    has children without BMO_NODE_SPLIT).  (ii) A GaussianBeamlet split BEFORE the end of its
                                    stored path: the children's w0 / E0 come from gauss_parameters(gauss, length(gauss)) with
                                    the stale tail still attached (ThinBeamsplitter.jl:125; the tail is cut after the loop,
                                    System.jl:417-421) — reproduced from the previous solution's segment log.
                                    (Rounds 1-3 dropped such children / sized them at the split and asked the wrapper to fall back.) */
};

/* ------------------------------------------------------------------ shapes */
enum bmo_shape_kind {
    BMO_SHAPE_MESH = 0,        /* src/Mesh.jl:33-39;  tri_begin/tri_count, world-space vertices   */
    BMO_SHAPE_SPHERE = 1,      /* SphericalLensSDF.jl:72-89   p = {radius}                         */
    BMO_SHAPE_PLANO = 2,       /* SphericalLensSDF.jl:41-65   p = {thickness, diameter}            */
    BMO_SHAPE_CONVEX = 3,      /* SphericalLensSDF.jl:186-232 p = {radius, diameter, sag, height}  */
    BMO_SHAPE_CONCAVE = 4,     /* SphericalLensSDF.jl:131-170 p = {radius, diameter, sag}          */
    BMO_SHAPE_UNION = 5,       /* UnionSDF.jl:22-91           children                             */
    BMO_SHAPE_BOX = 6,         /* PrimitiveSDF.jl:13-46       p = {hx, hy, hz} half edge lengths   */
    BMO_SHAPE_CYLINDER = 7,    /* PrimitiveSDF.jl:53-76       p = {radius, height}                 */
    BMO_SHAPE_CUTSPHERE = 8,   /* PrimitiveSDF.jl:83-124      p = {radius, height, w}              */
    BMO_SHAPE_RING = 9,        /* PrimitiveSDF.jl:132-166     p = {inner_radius, hwidth, hthickness} */
    BMO_SHAPE_PRISM = 10,      /* PrimitiveSDF.jl:183-210     p = {hx, hy, hz}                     */
    BMO_SHAPE_MENISCUS = 11,   /* MeniscusLensSDF.jl:19-46    children = {convex, cylinder, concave} in the meniscus frame */
    BMO_SHAPE_POINT = 12,      /* test/runtests.jl:926-947 TestPointSDF: sdf = norm(p)             */
    BMO_SHAPE_ASPH_CONVEX = 13,  /* AsphericalLensSDF.jl:19-28,309-327  p = {radius, conic, diameter, max_sag}; coefs = child range */
    BMO_SHAPE_ASPH_CONCAVE = 14, /* AsphericalLensSDF.jl:85-96,329-349  p = {radius, conic, diameter, max_sag}; coefs = child range */
    BMO_SHAPE_CYL_CONVEX = 15,   /* CylindricalSDF.jl:25-85   p = {radius, diameter, height}           */
    BMO_SHAPE_CYL_CONCAVE = 16,  /* CylindricalSDF.jl:92-139  p = {radius, diameter, height}           */
    BMO_SHAPE_ACYL_CONVEX = 17,  /* AcylindricalSDF.jl:16-74   p = {radius, diameter, height, conic, max_sag}; coefs = child range */
    BMO_SHAPE_ACYL_CONCAVE = 18, /* AcylindricalSDF.jl:83-141  p = {radius, diameter, height, conic, max_sag}; coefs = child range */
    BMO_SHAPE_KIND_COUNT
};

#define BMO_SHAPE_NPARAM 8
/* The SDF is a first-order distance ESTIMATE (aspheres: |z - z(r)| / |grad|), not 1-Lipschitz: only the bounding-sphere
 * culls apply to it, not the running-t prune nor the union child skip (DESIGN.md "miss cull").  Unions inherit it. */
#define BMO_SHAPE_FLAG_INEXACT 1
/* Library-internal (set by bmo_scene_create on its own copy of the tables, ignored on input): the children of this UNION are
 * consecutive shape ids starting at tri_begin (unused by unions otherwise), so the walk over children needs no children[] read. */
#define BMO_SHAPE_FLAG_CONSECUTIVE 2
/* Input: keep brute force (every face, every ray) for this MESH even above BMO_MESH_BVH_MIN_FACES. */
#define BMO_SHAPE_FLAG_NO_BVH 4
/* Library-internal (set by bmo_scene_create on its own copy of the tables, ignored on input): this MESH is traced through a bounding
 * volume hierarchy; child_begin (unused by meshes otherwise) holds the index of its first node.  The BVH returns the same face as the
 * brute-force loop of Mesh.jl:244-267, bit for bit (DESIGN.md §3 "mesh BVH"). */
#define BMO_SHAPE_FLAG_BVH 8
/* A MESH with at least this many faces (and without BMO_SHAPE_FLAG_NO_BVH) gets a BVH. */
#define BMO_MESH_BVH_MIN_FACES 64

typedef struct bmo_shape {
    int32_t kind;
    int32_t child_begin;   /* UNION, MENISCUS: index into bmo_scene_desc.children;
                              ASPH_*: index into bmo_scene_desc.coefs (even aspheric coefficients A4, A6, ...) */
    int32_t child_count;
    int32_t tri_begin;     /* MESH: first triangle                                   */
    int32_t tri_count;
    int32_t flags;         /* BMO_SHAPE_FLAG_* */
    double pos[3];         /* position(shape)                                        */
    double dir[9];         /* orientation(shape), row-major 3x3                      */
    double tdir[9];        /* transposed_orientation(shape) (AbstractSDF.jl:20-27), row-major;
                              identity for SPHERE (SphericalLensSDF.jl:82-84)        */
    double p[BMO_SHAPE_NPARAM];
    /* Conservative world-space bounding sphere, used ONLY for the provably
       equivalent miss shortcut (DESIGN.md "miss cull"); radius < 0 disables it. */
    double bs_center[3];
    double bs_radius;
} bmo_shape;

/* ----------------------------------------------------------------- objects */
enum bmo_object_kind {
    BMO_OBJ_MIRROR = 0,          /* AbstractReflectiveOptic   Mirrors.jl:39-69                    */
    BMO_OBJ_REFRACTIVE = 1,      /* Lens / Prism              Lenses.jl:46-126                    */
    BMO_OBJ_DOUBLET = 2,         /* DoubletLens               DoubletLenses.jl:26-76  shape={front,back} medium={n1,n2} */
    BMO_OBJ_THIN_BS = 3,         /* ThinBeamsplitter          ThinBeamsplitter.jl:16-168          */
    BMO_OBJ_PLATE_BS = 4,        /* plate splitter            PlateBeamsplitter.jl:160-275 shape={substrate,coating}    */
    BMO_OBJ_CUBE_BS = 5,         /* cube splitter             CubeBeamsplitter.jl:63-121   shape={front,back,coating}   */
    BMO_OBJ_SPOTDETECTOR = 6,    /* Spotdetector.jl:50-61                                         */
    BMO_OBJ_PSFDETECTOR = 7,     /* PSFDetector.jl:77-89                                          */
    BMO_OBJ_INTERSECTABLE = 8,   /* Intersectable.jl:15                                           */
    BMO_OBJ_NONINTERACTABLE = 9, /* NonInteractable.jl:19-20                                      */
    BMO_OBJ_POLARIZER = 10,      /* PolarizationFilter.jl:31-48                                   */
    BMO_OBJ_PHOTODETECTOR = 11,  /* Detectors/Photodetector.jl:57-107: a GaussianBeamlet that hits it stops and is
                                    recorded in the detector slot (3 hit rows per beamlet, row 0 = {proj, 0...});
                                    the complex field is read out with bmo_photodetector_field.  Ray / PolarizedRay
                                    beams stop without a record (Photodetector.jl:57-60 warns)              */
    BMO_OBJ_KIND_COUNT
};

typedef struct bmo_object {
    int32_t kind;
    int32_t shape[3];      /* part shapes, -1 when unused (see kind)                 */
    int32_t medium[2];     /* rows of n_table for refractive parts, -1 when unused   */
    int32_t detector;      /* detector slot (0..n_detectors-1) or -1                 */
    int32_t reserved;
    double reflectance;    /* amplitude R (ThinBeamsplitter.jl:47-50)                */
    double transmittance;  /* amplitude T                                            */
    double cutoff;         /* PolarizationFilter cutoff                              */
    double jones[18];      /* GlobalJonesBasis 3x3 complex, row-major (re,im) pairs  */
} bmo_object;

/* ------------------------------------------------------------------- scene */
typedef struct bmo_scene_desc {
    int32_t abi_version;   /* BMO_ABI_VERSION */
    int32_t n_objects;     /* leaf objects in Leaves() order (System.jl:21)          */
    int32_t n_shapes;
    int32_t n_children;
    int32_t n_tris;
    int32_t n_media;
    int32_t n_lambda;
    int32_t n_detectors;
    const bmo_object* objects;
    const bmo_shape* shapes;
    const int32_t* children;  /* shape ids                                           */
    const double* tris;       /* 9 doubles per triangle: V1 V2 V3 (world space)      */
    const double* n_table;    /* [n_media][n_lambda]: n_obj(lambda) evaluated by the host
                                 (RefractiveIndexUtils.jl functors cannot cross a C ABI) */
    const double* lambdas;    /* [n_lambda] distinct wavelengths of the batch        */
    const double* coefs;      /* [n_coefs] pooled aspheric coefficients              */
    /* tracing constants; the reference's compile-time values are the defaults */
    double eps_srf;        /* 1e-9  AbstractSDF.jl:1  */
    double eps_ray;        /* 1e-10 AbstractSDF.jl:2  */
    double eps_ins;        /* 1.0   AbstractSDF.jl:3  */
    double mt_keps;        /* 1e-9  Mesh.jl:203       */
    double mt_leps;        /* 1e-9  Mesh.jl:203       */
    double grad_h;         /* 1e-8  AbstractSDF.jl:83 */
    int32_t march_iters;   /* 1000  AbstractSDF.jl:105,135 */
    int32_t n_coefs;
} bmo_scene_desc;

typedef struct bmo_scene bmo_scene; /* opaque, immutable after create, shareable */

/* ------------------------------------------------------------------- beams */
enum bmo_beam_kind {
    BMO_BEAM_RAY = 0,        /* Beam{T,Ray{T}}           Rays.jl:14-20        */
    BMO_BEAM_POLARIZED = 1,  /* Beam{T,PolarizedRay{T}}  PolarizedRays.jl:37-66 */
    BMO_BEAM_GAUSSIAN = 2    /* GaussianBeamlet          Gaussian.jl:33-42    */
};

/* Planar (structure-of-arrays) input: plane i occupies planes[i*n .. (i+1)*n).
 *   RAY        (8 planes):  px py pz dx dy dz lambda n
 *   POLARIZED  (14 planes): the 8 above, then Re(E0x) Im(E0x) Re(E0y) Im(E0y) Re(E0z) Im(E0z)
 *   GAUSSIAN   (25 planes): chief px..dz (6), waist px..dz (6), divergence px..dz (6),
 *                           lambda, n, w0, Re(E0), Im(E0), then 2 reserved (0)
 *              (31 planes): the 25 above, then lenA lenB l0 oplC oplW oplD — the lengths a SOLVED beamlet has accumulated up to the
 *                           segment this batch continues (solve_system!(...; retrace = false) on beamlets whose last ray is open,
 *                           System.jl:449-458): lenA = sum of the chief's own earlier segment lengths folded from 0
 *                           (length_rays, Beam.jl:160-169), lenB = the same fold started from l0, l0 = length(parent chief beam)
 *                           (Beam.jl:125-130; 0 for a root), oplC = optical path of the chief, parents included, oplW / oplD =
 *                           optical path of the waist / divergence beams' own earlier segments (Beam.jl:137-149)
 * dir must already be normalised by the caller exactly as the Ray constructor does
 * (Rays.jl:32-42); the engine does not renormalise first segments.               */
#define BMO_PLANES_RAY 8
#define BMO_PLANES_POLARIZED 14
#define BMO_PLANES_GAUSSIAN 25
#define BMO_PLANES_GAUSSIAN_CONTINUED 31

typedef struct bmo_ray_batch {
    int64_t n;                  /* number of root beams                              */
    int32_t kind;               /* bmo_beam_kind                                     */
    int32_t n_planes;
    const double* planes;       /* host pointer, n_planes * n doubles                */
    const int32_t* lambda_idx;  /* [n] index of each beam's wavelength in lambdas    */
} bmo_ray_batch;

typedef struct bmo_trace_opts {
    int32_t r_max;              /* solve_system! default 100 (System.jl:444)         */
    int32_t device;             /* HIP device ordinal                                */
    int32_t record_segments;    /* 1: keep the full segment log (reference behaviour).  0: keep only the beam tree, statuses,
                                   counts and detector hits - a solve then holds three bounce levels in HBM instead of all
                                   of them (8x less on config C2), for spot diagrams / PSFs of very large bundles; the view of
                                   such a result reports n_records = 0, and it cannot be retraced or read out as a
                                   Photodetector field (both need the segments): BMO_ERR_INVALID.                     */
    int32_t max_beams;          /* 0: no limit (reference behaviour).  > 0: stop with BMO_ERR_LIMIT once the solve holds more
                                   than this many beams (tree nodes).  A splitter facing a mirror multiplies beams on every
                                   pass; solve_system! recurses until memory runs out on such a system, and so does this
                                   library (BMO_ERR_OOM after filling HBM) unless a limit is set.                      */
} bmo_trace_opts;

/* ------------------------------------------------------------------ result
 * All arrays are owned by the result handle until bmo_result_free.  Nodes are
 * beam-tree nodes (one Beam / GaussianBeamlet each) in REFERENCE order: bundle
 * order, and inside one root's tree the BFS order of solve_system! (System.jl:446-458,
 * transmitted child before reflected child, Beamsplitters.jl:16-19).  Records are
 * ray segments grouped by node in that order, k = 0..nseg-1 inside a node.
 * Planes per record:
 *   RAY:       px py pz dx dy dz n | t nx ny nz                       (11)
 *   POLARIZED: the 11 above, then Re/Im E0x E0y E0z                   (17)
 *   GAUSSIAN:  chief(11) waist(11) divergence(11)                     (33)
 * A record whose ray has no intersection has obj = shape = -1, t = +Inf.          */
typedef struct bmo_trace_result_view {
    int64_t n_roots;
    int64_t n_nodes;
    int64_t n_records;
    int64_t n_intersect_calls;  /* intersect3d(object|hint shape, ray) calls the reference
                                   algorithm performs for this trace (BASELINE metric) */
    int32_t n_steps;            /* step-kernel launches (each advances every active beam by up to 32 bounces) */
    int32_t beam_kind;
    int32_t rec_planes;         /* planes per record                                 */
    int32_t n_detectors;
    const int32_t* node_root;
    const int32_t* node_parent;       /* node index or -1                            */
    const int32_t* node_first_child;  /* node index of transmitted child (+1 = reflected) or -1 */
    const int32_t* node_first_rec;    /* first record of the node                    */
    const int32_t* node_nseg;         /* length(rays(beam))                          */
    const int32_t* node_status;       /* bmo_node_status bits                        */
    const double* node_aux;           /* [n_nodes*4]: GAUSSIAN w0, Re(E0), Im(E0), lambda; else lambda,0,0,0 */
    const int32_t* rec_obj;           /* Intersection.object as leaf index           */
    const int32_t* rec_shape;         /* Intersection.shape as shape id              */
    const double* rec;                /* planar [rec_planes][n_records]              */
    /* detector hit lists in reference push! order */
    const int64_t* det_count;         /* [n_detectors]                               */
    const int64_t* det_offset;        /* [n_detectors] offset into det_data (in hits) */
    const int32_t* det_node;          /* [total hits] node that produced the hit     */
    const double* det_data;           /* [total hits][9]: Spot: x z 0..; PSF: hit(3) dir(3) opl proj k */
} bmo_trace_result_view;

typedef struct bmo_trace_result bmo_trace_result; /* opaque */

/* ---------------------------------------------------------------- functions */
int bmo_version(void);
const char* bmo_last_error(void);
/* SHA-256 (hex) of the engine sources this library was built from (csrc/bmo_engine.hip, bmo_lane.hpp, bmo_readout.inc.hpp and this
   header, in that order), recorded by the build; "" for a build that did not record one.  The host side compares it with the sources
   it finds next to the library and refuses a stale binary (there is no reference counterpart: housekeeping of the boundary). */
const char* bmo_source_hash(void);
/* First 16 hex digits of the SHA-256 of the compiler flag list the library was built with (__graft_entry__.HIP_FLAGS joined by
   blanks); "" for a build that did not record one.  Bit-level parity with the reference depends on some of those flags
   (-ffp-contract=off: Julia never contracts a*b+c), so the host side refuses a library built with other flags, like a stale one. */
const char* bmo_build_flags_hash(void);

/* Number of usable HIP devices (0 = none). */
int bmo_device_count(void);

/* Device self-test of the scalar rules of the lane code as the device compiler built them: Base.max / Base.min for Float64 (NaN if
   either operand is NaN, -0.0 < +0.0; the AbstractSDF leaf formulas) written without control flow against the rule written with compares,
   their ForwardDiff.Dual forms (selection: the winner's value and partials, ties to the second argument) and abs(::Dual), bit for bit over
   every pair of a table of special values (zeros, denormals, infinities, NaN, ordinary numbers); then the elementary functions of
   csrc/bmo_jlmath.hpp on ~7 000 arguments against the host build of the same code.  BMO_OK, or BMO_ERR_INTERNAL with the first mismatch
   in bmo_last_error(). */
int bmo_selftest(int32_t device);

/* The elementary functions of the step path as the engine evaluates them (csrc/bmo_jlmath.hpp: Julia Base's sin / cos / tan / acos / atan —
   base/special/trig.jl, rem_pio2.jl — restated; the reference calls them in OpticUtils.jl:121-131, LinearAlgebraUtils.jl:103-108,
   Gaussian.jl:326-345), host build, one value per call: which = 0 sin(x), 1 cos(x), 2 tan(x), 3 acos(x), 4 atan(x), 5 atan(y, x).  For a
   maintainer to compare with Base itself; bmo_selftest compares the device's results with these.  NaN for another `which`. */
double bmo_jl_trig(int32_t which, double x, double y);

int bmo_scene_create(const bmo_scene_desc* desc, bmo_scene** out);
/* BVH of mesh shape `shape` as bmo_scene_create built it: node count (0: the shape is traced by brute force), depth (root = 1) and the
   largest leaf (faces).  BMO_ERR_INVALID for a bad id.  No GPU needed. */
int bmo_scene_mesh_bvh(const bmo_scene* scene, int32_t shape, int32_t* n_nodes, int32_t* depth, int32_t* max_leaf);
/* Check entry: intersect3d(mesh, ray) of mesh shape `shape` for n rays (pos / dir: n x 3, row-major) evaluated on the host by the
   engine's own lane code against the scene blob the GPU reads — the BVH traversal for a shape with a BVH, the brute-force loop
   otherwise.  t[i]: the hit's t (+Inf: none), fid[i]: the face (0-based within the mesh, -1: none).  No GPU needed. */
int bmo_mesh_nearest_host(const bmo_scene* scene, int32_t shape, int64_t n, const double* pos, const double* dir, double* t, int32_t* fid);
int bmo_scene_destroy(bmo_scene* scene);
/* The engine keeps freed device blocks in a per-device pool for reuse by the next trace; this returns them to HIP. */
int bmo_pool_release(void);

/* One call = solve_system!(system, group; r_max) for a fresh (un-solved) batch:
 * upload, trace on the device, canonicalise, download.                            */
int bmo_trace(bmo_scene* scene, const bmo_ray_batch* in, const bmo_trace_opts* opts,
              bmo_trace_result** out);

/* Split form used by benchmarks and multi-GPU drivers: inputs stay resident in HBM. */
typedef struct bmo_device_batch bmo_device_batch; /* opaque */
int bmo_batch_upload(bmo_scene* scene, const bmo_ray_batch* in, int32_t device, bmo_device_batch** out);
int bmo_batch_free(bmo_device_batch* batch);
/* Runs the whole trace on the device (all bounce steps, child spawning, detector
 * hit compaction + ordering).  Results stay on the device inside *out; blocks until done. */
int bmo_trace_device(bmo_scene* scene, bmo_device_batch* batch, const bmo_trace_opts* opts,
                     bmo_trace_result** out);
/* Device pointers of the ordered detector hit buffers (for RCCL all-gather):
 * data = [count][9] doubles on the device the trace ran on.                        */
int bmo_result_device_hits(bmo_trace_result* res, int32_t detector, const double** data, int64_t* count);
/* Copies up to max_hits ordered hits (9 doubles each) of one detector into dst: a pointer on the device the
 * trace ran on (e.g. the data_ptr of a torch tensor used as RCCL all-gather input) or host memory (page-locked
 * memory copies at PCIe speed; pageable memory works, slower) - the Spotdetector read-out that does not need
 * the segment log.                                                                                          */
int bmo_result_copy_hits(bmo_trace_result* res, int32_t detector, double* dst, int64_t max_hits);
/* Kernel timing of the last trace: sum over step-kernel launches, HIP events on the trace stream. */
int bmo_result_timing(bmo_trace_result* res, double* step_kernel_ms, double* total_ms, int32_t* n_launches);
/* Size of the solution without downloading it: reference intersect3d calls, segments, beams (tree nodes), detector hits. */
int bmo_result_counts(bmo_trace_result* res, int64_t* n_intersect_calls, int64_t* n_records, int64_t* n_nodes, int64_t* n_hits);
/* Materialise host views (downloads + canonical ordering of the segment log): the whole solution, i.e.
 * bmo_result_view_select(res, BMO_VIEW_HITS | BMO_VIEW_SEGMENTS, view). */
int bmo_result_view(bmo_trace_result* res, bmo_trace_result_view* view);
/* Selective view: the wrapper that only needs what the reference's users usually read after solve_system! —
 * last(rays(beam)) (src/Beam.jl:79), the beam tree (src/AbstractTypes/AbstractBeam.jl:48-78) and the detectors' data
 * (Spotdetector.jl:27, PSFDetector.jl:57) — does not pay for the segment log (3.7 GB per solve of config C2 over PCIe).
 * The node tables (node_*) are always filled.  `what` is a mask of:
 *   BMO_VIEW_HITS          det_node / det_data (det_count / det_offset are always valid)
 *   BMO_VIEW_LAST_SEGMENT  rec / rec_obj / rec_shape hold ONE record per beam, its last ray segment: n_records = n_nodes and
 *                          node_first_rec[i] = i, while node_nseg[i] stays the beam's true length(rays(beam))
 *   BMO_VIEW_SEGMENTS      the whole log (wins over BMO_VIEW_LAST_SEGMENT)
 * Without a record flag n_records = 0 and rec* = NULL.  Every part is downloaded once per result and kept in page-locked
 * host memory; asking for BMO_VIEW_SEGMENTS after BMO_VIEW_LAST_SEGMENT replaces the record tables (earlier views' rec*
 * pointers die), asking for BMO_VIEW_LAST_SEGMENT alone after the whole log is BMO_ERR_INVALID (the log already has it).
 * A view may be taken from another host thread while the next solve of another result runs: its kernels and copies go to
 * the NULL stream, which does not synchronise with the library's (non-blocking) trace stream. */
#define BMO_VIEW_HITS 1u
#define BMO_VIEW_LAST_SEGMENT 2u
#define BMO_VIEW_SEGMENTS 4u
int bmo_result_view_select(bmo_trace_result* res, uint32_t what, bmo_trace_result_view* view);
/* bmo_result_copy_hits for the leading n_cols (1..9) columns only, packed [hits][n_cols]: a Spotdetector keeps x, y
 * (Spotdetector.jl:59), so the multi-GPU all-gather moves 16 B per hit instead of 72.  dst: device or host memory. */
int bmo_result_copy_hit_columns(bmo_trace_result* res, int32_t detector, int32_t n_cols, double* dst, int64_t max_hits);
int bmo_result_free(bmo_trace_result* res);

/* ------------------------------------------------------------------------------------------------
 * Retracing: the second and later solve_system!(system, beams) on already solved beams —
 * retrace_system! src/System.jl:188-255 (Beam), :326-428 (GaussianBeamlet), driven by solve_system! :444-461.
 *
 * `prev` is the result of the previous solve of the SAME beams (bmo_trace*, or an earlier bmo_retrace*); it stays valid and
 * is not modified.  `scene` is the system as it is now (elements moved by the caller): it must have the object and shape
 * numbering `prev` was solved with.  The batch supplies the root heads (first ray of every root beam; for Gaussian beamlets
 * also lambda, w0, E0) and must have prev's root count and beam kind.
 *
 * Every stored ray is re-intersected with the object of its stored intersection only (or with the shape hinted by the
 * preceding interaction), interacted, and the following stored ray is overwritten (replace!, Beam.jl:81-94); where the
 * stored path ends or breaks the beam is cut, its children are dropped and normal tracing continues without a hint.
 * Splitter children of an intact parent keep their identity and are re-walked with heads rewritten by the parent
 * (children!, AbstractBeam.jl:62-76; a Gaussian child keeps its stored w0, Gaussian.jl:154-161).
 * The result has the layout of a fresh trace.  n_intersect_calls counts the reference's intersect3d calls (one per
 * re-walked ray and sub-ray, plus those of the continued trace).                                                     */
int bmo_retrace(bmo_scene* scene, const bmo_ray_batch* in, bmo_trace_result* prev, const bmo_trace_opts* opts, bmo_trace_result** out);
int bmo_retrace_device(bmo_scene* scene, bmo_device_batch* batch, bmo_trace_result* prev, const bmo_trace_opts* opts,
                       bmo_trace_result** out);

/* ------------------------------------------------------------------------------------------------
 * Detector read-out: intensity(psf::PSFDetector) — src/OpticalComponents/Detectors/PSFDetector.jl:190-237.
 *
 *   field(i,j) = sum over hits h of  proj_h * cis(k_h * (opl_h + dot(p_ij - hit_h, dir_h))),   p_ij = origin + xs[i]*e1 + zs[j]*e2
 *   intensity  = abs2(field)                       (raw / unscaled, as the reference returns it)
 *
 * hits    : [n_hits][9] doubles (hit xyz, dir xyz, opl, proj, k) — the PSF rows of bmo_trace_result_view::det_data or the
 *           device pointer of bmo_result_device_hits (hits_on_device != 0: pointer on `device`).
 * xs, zs  : the n sample coordinates of the detector-local x and z axes (host arrays; the reference's LinRange + shift).
 * out_intensity : host, n*n doubles, element (i,j) at [i + n*j]  (Julia's column-major Matrix).
 * out_field     : optional host buffer, n*n complex values as (re, im) pairs, same order; may be NULL.
 * kernel_ms     : optional; HIP-event time of the accumulation kernels.
 * The sum over hits is evaluated in a fixed blocked order (deterministic, but not the reference's sequential order):
 * parity with the reference is to the floating-point tolerance of a re-associated sum, not bit-exact.            */
int bmo_psf_intensity(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                      const double e2[3], const double* xs, const double* zs, int32_t n, int32_t device, double* out_intensity,
                      double* out_field, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Photodetector field: interact3d(::Photodetector, ::GaussianBeamlet, ray_id) —
 * src/OpticalComponents/Detectors/Photodetector.jl:69-107 with electric_field(gauss, r, z) src/Gaussian.jl:381-392,
 * gauss_parameters :298-353, point_on_beam src/Beam.jl:177-205, electric_field(r, z, ...) src/Utils/OpticUtils.jl:87-89.
 *
 * For every beamlet of `res` recorded on detector slot `detector` (reference order) and every grid point (i, j):
 *   p1 = position + xs[i]*orientation[:,1] + ys[j]*orientation[:,3]      (written out per component like the reference)
 *   l1 = dot(p1 - p0, d0);  r = |p1 - (p0 + l1*d0)|;  z = l0 + l1       (p0, d0: last chief ray; l0 = length up to it)
 *   field(i,j) += electric_field(gauss, r, z) * sqrt(proj)
 * The reference does this inside solve_system!; here the trace only records the hit and this call evaluates the sum on the
 * GPU from the segment log still resident in `res` (any segment of the beamlet may be selected by point_on_beam).
 *
 * position / orientation : the detector's pose (orientation row-major 3x3, columns = local axes) at solve time.
 * xs[nx], ys[ny]         : local sample coordinates (the reference's LinRange pd.x, pd.y).
 * field_inout            : host, nx*ny complex values as (re, im) pairs, element (i,j) at [i + nx*j]; contributions are ADDED
 *                          (the reference accumulates until empty!(pd)).
 * The sum over beamlets is evaluated in a fixed blocked order: parity with the reference is to FP64 re-association
 * tolerance, not bit-exact.                                                                                          */
int bmo_photodetector_field(bmo_trace_result* res, int32_t detector, const double position[3], const double orientation[9], const double* xs,
                            const double* ys, int32_t nx, int32_t ny, double* field_inout, double* kernel_ms);

/* gauss_parameters(gauss, z) — src/Gaussian.jl:298-353 with point_on_beam src/Beam.jl:177-205 — for ONE solved beamlet of `res`
 * (index in the result's node order) at n distances z along the beam (measured like the reference's: from the start of the root
 * beamlet, parents included): out[4*i .. 4*i+3] = w (local radius), R (wavefront curvature 1/r), psi (Gouy phase), w0 (local waist).
 * Evaluated on the GPU by the code bmo_photodetector_field runs per grid point; exists so that the reference's Gaussian
 * known-answer tests (test/runtests.jl:1811-1932) can be run against the device arithmetic itself.                         */
int bmo_gauss_parameters(bmo_trace_result* res, int64_t node, const double* zs, int32_t n, double* out);

/* Earlier segments of CONTINUED GaussianBeamlets — solve_system!(system, beams; retrace = false) on beamlets solved before traces their
 * open last rays on (src/System.jl:449-458, solve_leaf! :470-475); `res` is the solution of such a continuation (root beamlet i = the
 * i-th continued beamlet from its open ray on, bmo.h "31 planes").  gauss_parameters and the Photodetector field of a beamlet are
 * functions of ALL its rays (point_on_beam, length, optical_path_length: src/Beam.jl:125-205), so the rays in front of the open one are
 * handed over here before bmo_photodetector_field / bmo_gauss_parameters are called on `res`:
 *   prefix_start[n_roots + 1] : exclusive scan of the number of earlier segments per root beamlet (0 for a beamlet without any);
 *   prefix_segs[24][total]    : plane 8 b + q of segment s at [(8 b + q) * total + s]; b = chief, waist, divergence;
 *                               q = pos 0-2, dir 3-5, refractive index 6, length t 7;   total = prefix_start[n_roots];
 *   opl_parent[n_roots]       : optical_path_length(parent(chief beam)), 0 without a parent.
 * The tables are copied to the device and replace an earlier prefix of `res`.  n_roots must be the root count of `res`.        */
int bmo_result_set_gauss_prefix(bmo_trace_result* res, int64_t n_roots, const int32_t* prefix_start, const double* prefix_segs, const double* opl_parent);

/* ------------------------------------------------------------------------------------------------
 * Sweeps (DESIGN.md §3 "Sweeps"): many configurations of one system, solved in one call.  The reference's scans — move an element,
 * solve_system!, read a detector, repeat (docs/src/tutorials/michelson.md "Running successive simulations", test/runtests.jl:2092-2121) —
 * become one trace whose root beams each belong to one configuration.
 *
 * A configuration is a snapshot of the same system after the caller's kinematics or parameter changes.  All configurations share the
 * topology: counts, object and shape kinds, part shape ids, media ids, detector slots, child structure, triangle ranges, shape flags,
 * wavelengths and tracing constants.  The numbers may differ: poses, bounding spheres, shape parameters, vertices, object constants and
 * n_table values.
 *
 * bmo_scene_create_sweep validates that (BMO_ERR_INVALID naming the first field that differs from configuration 0; no GPU needed) and lays
 * the configurations out at the same offsets, one `stride` apart (the mesh BVH tables sized to the largest configuration's).  Every
 * configuration is a full copy of the scene tables.  bmo_scene_destroy frees the handle.  bmo_trace / bmo_batch_upload / bmo_trace_device /
 * bmo_retrace* refuse a sweep scene of more than one configuration (BMO_ERR_INVALID); bmo_scene_mesh_bvh and bmo_mesh_nearest_host describe
 * configuration 0.
 *
 * bmo_trace_sweep: root i belongs to configuration root_config[i], non-decreasing, in [0, n_configs) (BMO_ERR_INVALID otherwise, checked
 * before a device is looked for).  The result is an ordinary bmo_trace_result: nodes in reference order, so every configuration's beams and
 * detector hits are contiguous ranges.  Semantics: the slice of configuration c equals, bit for bit, a fresh bmo_trace of configuration c
 * on its roots — a FRESH solve of every configuration, not the reference's chain of retraces where step i re-walks step i - 1's solution
 * (the two agree where the scan keeps every beam on its path).  A sweep result cannot be retraced (BMO_ERR_UNSUPPORTED).
 * n_intersect_calls is the sum over all configurations.
 *
 * bmo_photodetector_field_sweep: the Photodetector field of every configuration in one set of launches.  positions [n_configs][3],
 * orientations [n_configs][9] (each as in bmo_photodetector_field), one grid xs / ys for all; field_inout [n_configs][nx*ny] (re, im) pairs,
 * contributions ADDED.  Configuration c sums only its own beamlets, in the blocked order bmo_photodetector_field uses for a solve that holds
 * only them: its field equals that call's bit for bit.  n_configs must be the sweep's.
 *
 * bmo_psf_intensity_sweep: the PSF intensity (bmo_psf_intensity) of every configuration in one set of launches, from the rows of the
 * PSFDetector slot `detector` still resident in `res`.  Configuration c samples its own axes xs[c][n], zs[c][n] at its own pose
 * (origins, e1s, e2s: [n_configs][3], as origin / e1 / e2 of bmo_psf_intensity).  out_intensity [n_configs][n*n], element (i,j) of
 * configuration c at [c*n*n + i + n*j]; out_field NULL or [n_configs][n*n] (re, im) pairs, same order.  Configuration c sums only its
 * own rows, split and summed in the blocked order bmo_psf_intensity uses for a call with exactly those rows: its intensity and field
 * equal that call's bit for bit.  A configuration without rows reads zero, as such a call with n_hits = 0 does.  n_configs must be the
 * sweep's, or 1 for an ordinary (non-sweep) result.  BMO_ERR_INVALID for a null pointer, n <= 0, a slot out of range or not a
 * PSFDetector's, or a wrong n_configs (all checked before a device is looked for); BMO_ERR_INTERNAL, never a wrong answer, if the rows of
 * a configuration are not consecutive.  kernel_ms: optional, HIP-event time of the accumulation and reduction launches.          */
int bmo_scene_create_sweep(const bmo_scene_desc* descs, int32_t n_configs, bmo_scene** out);
int bmo_trace_sweep(bmo_scene* sweep, const bmo_ray_batch* in, const int32_t* root_config, const bmo_trace_opts* opts, bmo_trace_result** out);
int bmo_photodetector_field_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* positions, const double* orientations,
                                  const double* xs, const double* ys, int32_t nx, int32_t ny, double* field_inout, double* kernel_ms);
int bmo_psf_intensity_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                            const double* e2s, const double* xs, const double* zs, int32_t n, double* out_intensity, double* out_field,
                            double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Spot read-out: the spot diagram of a Spotdetector (Spotdetector.jl:21-61 keeps the local x, z of every hit) as a binned image and as
 * moment statistics, computed on the device from the rows where they lie.  No reference counterpart: the reference's users bin and
 * average `sd.data` themselves.
 *
 * rows : [n_rows][row_cols] doubles, x in column 0 and z in column 1, row_cols in 2..9: the packed columns of bmo_result_copy_hit_columns,
 *        Spotdetector data, or the 9-column rows of bmo_result_device_hits (rows_on_device != 0: a pointer on `device`).
 * The _sweep forms read the rows of Spotdetector slot `detector` still resident in `res`, one image / one set of statistics per
 * configuration; n_configs must be the sweep's, or 1 for an ordinary (non-sweep) result.  They work on record_segments = 0 results (the
 * hit table is kept).  Configuration c is read exactly as the single call reads its rows: equal images, statistics equal bit for bit.
 *
 * Image, window (x0, x1, z0, z1), sx = nx / (x1 - x0) and sz = nz / (z1 - z0) computed once in FP64:
 *   a row is inside iff x >= x0 && x <= x1 && z >= z0 && z <= z1          (plain compares: a NaN is outside, the upper edge is closed)
 *   i = min((int64)floor((x - x0) * sx), nx - 1),  j likewise from z,  the row counts in image[i + nx * j]
 *   outside = rows that are not inside, so sum(image) + outside = n_rows.
 * image [n_configs][nx * nz], outside [n_configs], windows [n_configs][4].  Counts are integers: the image does not depend on the order
 * in which the device adds them.
 *
 * Statistics, stats [n_configs][BMO_SPOT_STAT_N] at the BMO_SPOT_STAT_* indices: the row count, the centroid, the extrema, the central
 * moments MXX = sum (x - cx)^2 / n, MZZ, MXZ about the COMPUTED centroid (two passes: sum x^2 - n cx^2 would lose every digit of a small
 * spot far off centre), RMS_R = sqrt(MXX + MZZ) and GEO_R = sqrt(max (x - cx)^2 + (z - cz)^2).  Count and extrema are exact; the sums run in
 * a fixed blocked order that depends on the row count only.  No rows: N = 0 and NaN in the other eleven; one row: moments and radii +0.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer, nx or nz <= 0 (or nx * nz >= 2^31), row_cols outside 2..9, a
 * window that is not finite or has not x1 > x0 and z1 > z0 (or whose extent has no finite bin width), a slot out of range or not a
 * Spotdetector's, a wrong n_configs.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result (no Spotdetector method for beamlets,
 * Spotdetector.jl:50; such slots hold three rows per beamlet).  kernel_ms: optional, HIP-event time of the launches.             */
enum bmo_spot_stat {
    BMO_SPOT_STAT_N_ROWS = 0, /* N: the row count                                  */
    BMO_SPOT_STAT_CX = 1,
    BMO_SPOT_STAT_CZ = 2,
    BMO_SPOT_STAT_X_MIN = 3,
    BMO_SPOT_STAT_X_MAX = 4,
    BMO_SPOT_STAT_Z_MIN = 5,
    BMO_SPOT_STAT_Z_MAX = 6,
    BMO_SPOT_STAT_MXX = 7,
    BMO_SPOT_STAT_MZZ = 8,
    BMO_SPOT_STAT_MXZ = 9,
    BMO_SPOT_STAT_RMS_R = 10,
    BMO_SPOT_STAT_GEO_R = 11
};
#define BMO_SPOT_STAT_N 12
int bmo_spot_image(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, const double window[4], int32_t nx,
                   int32_t nz, int32_t device, int64_t* image, int64_t* outside, double* kernel_ms);
int bmo_spot_image_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* windows, int32_t nx, int32_t nz,
                         int64_t* image, int64_t* outside, double* kernel_ms);
int bmo_spot_stats(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, int32_t device, double* stats,
                   double* kernel_ms);
int bmo_spot_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, double* stats, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Wavefront read-out: the scalar statistics of a PSFDetector's rows, computed on the device from the rows where they lie: the sampling
 * window of calc_local_lims (PSFDetector.jl:115-140), and the wavefront error and Strehl ratio that PSFDetector.jl:185-188 announces
 * ("a Strehl estimator will be added") but does not have.
 *
 * hits : [n_hits][9] doubles as for bmo_psf_intensity (hit xyz, dir xyz, opl, proj, k); origin, e1, e2 the detector pose as there.
 * ref_xz : the reference point (x, z) in detector-local coordinates, [2] (the _sweep form: [n_configs][2]); NULL: the centroid.
 * stats : [n_configs][BMO_PSF_STAT_N] at the BMO_PSF_STAT_* indices.  Everything is FP64, each expression evaluated left to right as
 * written, without contraction, h running over the rows:
 *   x_h = ((hx - ox) * e1x + (hy - oy) * e1y) + (hz - oz) * e1z,   z_h the same with e2                     (PSFDetector.jl:95-97)
 *   S = sum proj_h,   CX = (sum proj_h * x_h) / S,   CZ = (sum proj_h * z_h) / S                              (PSFDetector.jl:126-128)
 *   X_MIN .. Z_MAX, K_MIN, K_MAX: the extrema of x_h, z_h and k_h
 *   HWX = max |x_h - CX|,   HWZ = max |z_h - CZ|   about the COMPUTED centroid                                (PSFDetector.jl:135-136)
 *   (X_REF, Z_REF) = ref_xz or (CX, CZ);   p = (origin + X_REF * e1) + Z_REF * e2 per component   (the grid point of bmo_psf_intensity)
 *   l_h = ((px - hx) * dx + (py - hy) * dy) + (pz - hz) * dz,   W_h = opl_h + l_h,   phase_h = k_h * W_h      (PSFDetector.jl:229-230)
 *   W_MEAN = (sum proj_h * W_h) / S
 *   W_RMS = sqrt((sum proj_h * ((W_h - W_MEAN) * (W_h - W_MEAN))) / S)   in metres, about the computed mean in a pass of its own
 *   W_LO = min (W_h - W_MEAN),   W_HI = max (W_h - W_MEAN)                (peak-to-valley = W_HI - W_LO)
 *   F = sum proj_h * cis(phase_h)  (F_RE, F_IM: the field of bmo_psf_intensity at p),   STREHL = (F_RE * F_RE + F_IM * F_IM) / (S * S)
 * STREHL is the intensity at p over its value if every row arrived in phase: <= 1, rows of several wavelengths summed coherently as
 * intensity(psf) sums them.  No rows: N_ROWS = 0 and NaN in the other twenty.  The sums run in a fixed blocked order that depends on the
 * row count only (the order of bmo_spot_stats), so configuration c of the _sweep form equals the single call on its rows and resident
 * rows equal host rows, bit for bit.  The _sweep form reads the rows of PSFDetector slot `detector` still resident in `res` at the poses
 * origins / e1s / e2s [n_configs][3]; n_configs must be the sweep's, or 1 for an ordinary result; it works on record_segments = 0
 * results (the hit table is kept).
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer (ref_xz excepted), n_hits < 0, a slot out of range or not a
 * PSFDetector's, a wrong n_configs.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result (three rows per beamlet).  BMO_ERR_INTERNAL, never a
 * wrong answer, if the rows of a configuration are not consecutive.  kernel_ms: optional, HIP-event time of the launches.            */
enum bmo_psf_stat {
    BMO_PSF_STAT_N_ROWS = 0, /* N: the row count */
    BMO_PSF_STAT_S = 1,
    BMO_PSF_STAT_CX = 2,
    BMO_PSF_STAT_CZ = 3,
    BMO_PSF_STAT_X_MIN = 4,
    BMO_PSF_STAT_X_MAX = 5,
    BMO_PSF_STAT_Z_MIN = 6,
    BMO_PSF_STAT_Z_MAX = 7,
    BMO_PSF_STAT_HWX = 8,
    BMO_PSF_STAT_HWZ = 9,
    BMO_PSF_STAT_X_REF = 10,
    BMO_PSF_STAT_Z_REF = 11,
    BMO_PSF_STAT_W_MEAN = 12,
    BMO_PSF_STAT_W_RMS = 13,
    BMO_PSF_STAT_W_LO = 14,
    BMO_PSF_STAT_W_HI = 15,
    BMO_PSF_STAT_F_RE = 16,
    BMO_PSF_STAT_F_IM = 17,
    BMO_PSF_STAT_STREHL = 18,
    BMO_PSF_STAT_K_MIN = 19,
    BMO_PSF_STAT_K_MAX = 20
};
#define BMO_PSF_STAT_N 21
int bmo_psf_stats(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                  const double e2[3], const double* ref_xz, int32_t device, double* stats, double* kernel_ms);
int bmo_psf_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                        const double* e2s, const double* ref_xz, double* stats, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Zernike read-out: the least-squares Zernike coefficients of a PSFDetector's wavefront, computed on the device from the rows where they
 * lie: how much of the wavefront error of bmo_psf_stats is tilt, defocus, astigmatism, coma or spherical aberration.
 *
 * hits, origin, e1, e2, ref_xz, the _sweep form and its conventions: exactly those of bmo_psf_stats.
 * order : the highest radial order, 0 .. BMO_ZERNIKE_MAX_ORDER; J = (order + 1)(order + 2) / 2 terms (28 at most).
 * pupil : NULL or (U0, V0, RHO), [3] (the _sweep form: [n_configs][3]): centre and radius of the pupil in direction cosines.
 * coef  : [n_configs][J], metres.   info : [n_configs][BMO_ZERNIKE_INFO_N] at the BMO_ZERNIKE_* indices.
 * gram  : NULL or [n_configs][(J + 1)(J + 2) / 2], the packed lower triangle (row-major: entry (i, k), i >= k, at i (i + 1) / 2 + k) of the
 *         augmented normal equations below.
 * Everything is FP64, each expression evaluated left to right as written, without contraction, h running over the rows:
 *   X_REF, Z_REF, p, W_h, S, W_MEAN: as bmo_psf_stats defines them, the same expressions in the same blocked order: equal bit for bit.
 *   u_h = (dx * e1x + dy * e1y) + dz * e1z,   v_h the same with e2                  (the row's direction cosines in the detector frame)
 *   (U0, V0, RHO) = pupil, or U0 = (sum proj_h * u_h) / S,  V0 = (sum proj_h * v_h) / S,
 *                             RHO = sqrt(max_h ((u_h - U0) * (u_h - U0) + (v_h - V0) * (v_h - V0)))        about the computed centre
 *   x_h = (u_h - U0) / RHO,   y_h = (v_h - V0) / RHO,   t_h = x_h * x_h + y_h * y_h;   N_OUT = the rows with t_h > 1 (they are still fitted)
 *   Terms in OSA/ANSI order, j = (n (n + 2) + m) / 2 for n = 0 .. order, m = -n, -n + 2, .., n, in Cartesian form with +, -, * only:
 *     C_0 = 1, S_0 = 0, C_{k+1} = C_k * x - S_k * y, S_{k+1} = S_k * x + C_k * y                          (rho^k cos k theta, rho^k sin k theta)
 *     q_s, s = 0 .. K = (n - |m|) / 2: the integer coefficients of R_n^|m|(rho) / rho^|m| as a polynomial in t,
 *       q_s = (-1)^(K - s) (n - K + s)! / ((K - s)! ((n + |m|) / 2 - K + s)! s!);   Horner from the top: r = q_K; r = r * t + q_s, s = K - 1 .. 0
 *     Z_j = N * (r * A),  A = C_|m| for m >= 0 and S_|m| for m < 0,  N = sqrt((double)(n + 1)) for m = 0 and sqrt((double)(2 (n + 1)))
 *     otherwise (the correctly rounded root).  Z_0 evaluates to 1; the terms are orthonormal over the uniform unit disc.
 *   D_h = W_h - W_MEAN.  The fit minimises sum proj_h (D_h - sum_j c_j Z_j(x_h, y_h))^2.
 *   Augmented columns B_0 .. B_{J-1} = Z_j, B_J = D;  G_ik = sum_h (proj_h * B_i) * B_k for i >= k: the last row of `gram` holds the right
 *   hand side b_j = G_Jj and sum proj D^2.  Each entry's sum runs over the rows of a split in row order, the splits are folded in split
 *   order (the splits of bmo_spot_stats): a fixed order that depends on the row count only.
 *   Solve, a plain Cholesky factorisation G = L L^T of the J x J block, then two substitutions (sqrt and / IEEE):
 *     for j = 0 .. J-1:  d = G_jj;  for k = 0 .. j-1: d = d - L_jk * L_jk;   STATUS = 2 unless d > 0;   L_jj = sqrt(d);
 *                        for i = j+1 .. J-1:  s = G_ij;  for k = 0 .. j-1: s = s - L_ik * L_jk;   L_ij = s / L_jj
 *     for i = 0 .. J-1:  s = b_i;  for k = 0 .. i-1: s = s - L_ik * y_k;   y_i = s / L_ii
 *     for i = J-1 .. 0:  s = y_i;  for k = i+1 .. J-1: s = s - L_ki * c_k;   c_i = s / L_ii
 *   STATUS = 1, without solving, if N < J or RHO is zero or not finite; STATUS = 2 if a pivot is not > 0; for either, coef, FIT_RMS, E_LO
 *   and E_HI are NaN and the rest of info is still filled.
 *   F_h = ((c_0 * Z_0 + c_1 * Z_1) + ...) in ascending j,   E_h = D_h - F_h,   FIT_RMS = sqrt((sum proj_h * (E_h * E_h)) / S),
 *   E_LO = min E_h,  E_HI = max E_h.
 * No rows: N_ROWS = 0, STATUS = 1, NaN elsewhere (coef and gram too).  Configuration c of the _sweep form equals the single call on its
 * rows and resident rows equal host rows, bit for bit.  W_RMS is not repeated here: bmo_psf_stats has it.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than ref_xz, pupil, gram, kernel_ms; n_hits < 0; order
 * outside 0 .. BMO_ZERNIKE_MAX_ORDER; a given RHO that is not finite and > 0; a given U0 or V0 that is not finite; a slot out of range or
 * not a PSFDetector's; a wrong n_configs.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result.  BMO_ERR_INTERNAL, never a wrong answer, if the
 * rows of a configuration are not consecutive.  kernel_ms: optional, HIP-event time of the launches.                                 */
enum bmo_zernike_info {
    BMO_ZERNIKE_N_ROWS = 0, /* N: the row count */
    BMO_ZERNIKE_STATUS = 1, /* 0: solved, 1: not attempted, 2: a pivot was not > 0 */
    BMO_ZERNIKE_S = 2,
    BMO_ZERNIKE_X_REF = 3,
    BMO_ZERNIKE_Z_REF = 4,
    BMO_ZERNIKE_U0 = 5,
    BMO_ZERNIKE_V0 = 6,
    BMO_ZERNIKE_RHO = 7,
    BMO_ZERNIKE_W_MEAN = 8,
    BMO_ZERNIKE_FIT_RMS = 9,
    BMO_ZERNIKE_E_LO = 10,
    BMO_ZERNIKE_E_HI = 11,
    BMO_ZERNIKE_N_OUT = 12
};
#define BMO_ZERNIKE_INFO_N 13
#define BMO_ZERNIKE_MAX_ORDER 6
int bmo_psf_zernike(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                    const double e2[3], const double* ref_xz, const double* pupil, int32_t order, int32_t device, double* coef,
                    double* info, double* gram, double* kernel_ms);
int bmo_psf_zernike_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                          const double* e2s, const double* ref_xz, const double* pupil, int32_t order, double* coef, double* info,
                          double* gram, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * OPD map read-out: the wavefront of a PSFDetector's rows as a picture over the pupil, binned on the device from the rows where they lie:
 * the proj-weighted mean, per bin of an n x n grid over the pupil square, of the wavefront less a Zernike surface the caller chooses.
 *
 * hits, origin, e1, e2, ref_xz, pupil, the _sweep form and its conventions: exactly those of bmo_psf_zernike.
 * order : 0 .. BMO_ZERNIKE_MAX_ORDER, the order of the surface to remove; J = (order + 1)(order + 2) / 2.
 * coef  : [n_configs][J], metres: the Zernike surface that is REMOVED before binning (zero the terms to keep).  NULL only with order = 0,
 *         and then c_0 = 0: nothing is removed.
 * n     : bins per axis, 1 .. BMO_OPD_MAX_N.
 * opd, weight : [n_configs][n * n] doubles;  count : [n_configs][n * n] int64.  Bin (i, j) lies at i + n * j, i along u (x_h), j along v.
 * raw   : NULL or [n_configs][n * n][2] int64, the integer sums (Q_b, P_b) below.   info : [n_configs][BMO_OPD_INFO_N] at BMO_OPD_*.
 * Everything is FP64, each expression evaluated left to right as written, without contraction, h running over the N rows:
 *   X_REF, Z_REF, p, W_h, S, W_MEAN, u_h, v_h, (U0, V0, RHO), x_h, y_h, t_h, Z_j, F_h (with c = coef): as "Zernike read-out" defines them,
 *   the same expressions in the same blocked order of the sums: equal bit for bit.
 *   E_h = (W_h - W_MEAN) - F_h.   E_RMS, E_LO, E_HI, N_OUT: FIT_RMS, E_LO, E_HI and N_OUT of the Zernike read-out, the same expressions,
 *   record and fold: with coef, ref_xz = (X_REF, Z_REF) and pupil = (U0, V0, RHO) of a bmo_psf_zernike call on the same rows these four
 *   columns equal that call's bit for bit.
 *   Bins: the rule of bmo_spot_image on the window (-1, 1, -1, 1) of (x_h, y_h) with sx = n / 2.0: a row is inside iff
 *     x >= -1 && x <= 1 && y >= -1 && y <= 1 (plain compares: a NaN is outside, the upper edge is closed);
 *     i = min((int64)floor((x + 1.0) * sx), n - 1), j likewise with y.  N_OUTSIDE = the rows not inside; sum(count) + N_OUTSIDE = N.
 *     A row with t_h > 1 inside the square is binned, and counted in N_OUT.
 *   Fixed-point sums.  MQ = max_h |proj_h * E_h|, MP = max_h |proj_h| (each starts at 0; a row that compares false leaves it), N_BAD = the
 *     rows whose proj_h or proj_h * E_h is not finite.  b = the smallest integer with N <= 2^b.  For M in {MQ, MP}:
 *     sh(M) = 0 if M = 0, otherwise clamp(60 - b - ilogb(M), -1000, 1000);  SH_Q = sh(MQ), SH_P = sh(MP);  scale = ldexp(1.0, sh).
 *     q_h = (int64)rint((proj_h * E_h) * scale_q),  p_h = (int64)rint(proj_h * scale_p)  (ties to even);  |q_h| <= 2^(61 - b): the sum
 *     of a bin cannot leave int64.  Per bin b: count_b, Q_b = sum q_h, P_b = sum p_h over its rows, integer adds.
 *     weight_b = (double)P_b * ldexp(1.0, -SH_P);   opd_b = ((double)Q_b * ldexp(1.0, -SH_Q)) / weight_b, NaN where count_b = 0 or P_b = 0.
 *   The sums are integers: the maps do not depend on the order of the adds.  Configuration c of the _sweep form equals the single call on
 *   its rows and resident rows equal host rows, bit for bit, in every output.
 *   N_FILLED = the bins with count > 0;  MAP_LO, MAP_HI = the extrema of the opd_b that are not NaN, + 0.0 (a zero reads +0), NaN if none.
 * STATUS 0: read.
 * STATUS 1: no rows (N_ROWS = 0, NaN elsewhere in info), or RHO zero or not finite: no row is binned (count 0, opd and weight NaN, raw 0,
 *   N_OUTSIDE = N, N_FILLED = 0), E_RMS, E_LO, E_HI, SH_Q, SH_P, MAP_LO and MAP_HI are NaN, the rest of info is filled.
 * STATUS 2: N_BAD > 0: opd and weight are NaN, raw is 0, SH_Q, SH_P, MAP_LO and MAP_HI are NaN; count, N_OUTSIDE and N_FILLED are still
 *   exact, and E_RMS, E_LO, E_HI are what the Zernike read-out's expressions give on such rows.  Never a wrong answer.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than ref_xz, pupil, raw, kernel_ms and coef with order = 0;
 * n_hits < 0; n outside 1 .. BMO_OPD_MAX_N; order outside 0 .. BMO_ZERNIKE_MAX_ORDER; a NULL coef with order != 0; a given coef that is not
 * finite; the pupil, slot and n_configs refusals of bmo_psf_zernike.  BMO_ERR_LIMIT: the call's bin arrays ([n_configs][n * n] of Q, P and
 * count, 24 bytes a bin) would pass 4 GiB.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result.  A refused call writes nothing to the caller's
 * buffers.  kernel_ms: optional, HIP-event time of the launches.                                                                     */
enum bmo_opd_info {
    BMO_OPD_N_ROWS = 0,
    BMO_OPD_STATUS = 1, /* 0: read, 1: no rows or no usable RHO, 2: a row that is not finite */
    BMO_OPD_S = 2,
    BMO_OPD_X_REF = 3,
    BMO_OPD_Z_REF = 4,
    BMO_OPD_U0 = 5,
    BMO_OPD_V0 = 6,
    BMO_OPD_RHO = 7,
    BMO_OPD_W_MEAN = 8,
    BMO_OPD_E_RMS = 9,
    BMO_OPD_E_LO = 10,
    BMO_OPD_E_HI = 11,
    BMO_OPD_N_OUT = 12,
    BMO_OPD_N_OUTSIDE = 13,
    BMO_OPD_N_BAD = 14,
    BMO_OPD_N_FILLED = 15,
    BMO_OPD_SH_Q = 16,
    BMO_OPD_SH_P = 17,
    BMO_OPD_MAP_LO = 18,
    BMO_OPD_MAP_HI = 19
};
#define BMO_OPD_INFO_N 20
#define BMO_OPD_MAX_N 4096
int bmo_psf_opd_map(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                    const double e2[3], const double* ref_xz, const double* pupil, int32_t order, const double* coef, int32_t n,
                    int32_t device, double* opd, double* weight, int64_t* count, int64_t* raw, double* info, double* kernel_ms);
int bmo_psf_opd_map_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                          const double* e2s, const double* ref_xz, const double* pupil, int32_t order, const double* coef, int32_t n,
                          double* opd, double* weight, int64_t* count, int64_t* raw, double* info, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Through-focus read-out: the PSF of the same rows on a stack of displaced sample grids, and the spot statistics of the rows propagated to
 * a stack of planes, in one pass each over the rows where they lie.
 *
 * A PSF row carries its direction, so the field of bmo_psf_intensity at p + d depends on d through one factor per row:
 *   F_m(i,j) = sum_h proj_h * cis(k_h * (opl_h + dot(p_ij - hit_h, dir_h))) * cis(k_h * dot(d_m, dir_h))
 * which is what a PSFDetector translated by d_m and solved again reads (in a medium of index 1 the ray travels s further: hit' = hit + s dir,
 * opl' = opl + s, and k (opl' + dot(p + d - hit', dir)) is unchanged).  The first factor is the sincos per (row, point) of one plane; the
 * second is one sincos per (row, plane); a plane more costs one complex multiply-add per (row, point).
 *
 * bmo_psf_through_focus: hits, origin, e1, e2, xs, zs, n, device, kernel_ms as for bmo_psf_intensity.  displacements: [n_planes][3] world
 * vectors d_m (host).  out_intensity: host, [n_planes][n*n], plane m element (i,j) at [m*n*n + i + n*j]; out_field: optional, the same
 * order as (re, im) pairs.  FP64, no contraction, each expression left to right as written; per row r and point p = psf_point(xs[i], zs[j]):
 *   l = ((px - hx) * dx + (py - hy) * dy) + (pz - hz) * dz,   phase = k * (opl + l),   (s, c) = sincos(phase)     (bmo_psf_intensity's)
 *   t_re = proj * c,   t_im = proj * s
 *   g_m = (d_mx * dx + d_my * dy) + d_mz * dz,   (u_im, u_re) = sincos(k * g_m)
 *   re_m += t_re * u_re - t_im * u_im,   im_m += t_re * u_im + t_im * u_re
 * over the rows in the blocked order of bmo_psf_intensity for the same (n_hits, n): the plane with d_m = 0 has the factor (1, 0) and
 * equals bmo_psf_intensity's intensity bit for bit (its field as numbers: a zero may differ in sign).  n_hits = 0: zeros.
 *
 * bmo_psf_focus_stats: plane m is the detector plane moved to o_m = origin + offsets[m] * axis (per component), same e1, e2.  stats:
 * [n_planes][BMO_FOCUS_STAT_N] at the BMO_FOCUS_STAT_* indices.  Per row and plane, each expression left to right as written:
 *   nrm = e1 x e2   (nrm_x = e1y * e2z - e1z * e2y, nrm_y = e1z * e2x - e1x * e2z, nrm_z = e1x * e2y - e1y * e2x)
 *   den = (dx * nrm_x + dy * nrm_y) + dz * nrm_z
 *   s = (((omx - hx) * nrm_x + (omy - hy) * nrm_y) + (omz - hz) * nrm_z) / den
 *   q = hit + s * dir (per component)
 *   x = ((qx - omx) * e1x + (qy - omy) * e1y) + (qz - omz) * e1z,   z the same with e2
 *   S = sum proj,   CX = (sum proj * x) / S,   CZ = (sum proj * z) / S,   X_MIN .. Z_MAX the extrema of x and z           (first pass)
 *   ax = x - CX,  az = z - CZ about the COMPUTED centroid;   HWX = max |ax|,  HWZ = max |az|            (calc_local_lims at that plane)
 *   r2 = ax * ax + az * az,   RMS_R = sqrt((sum proj * r2) / S),   MAX_R = sqrt(max r2)                                 (second pass)
 * The sums run in the blocked order of bmo_psf_stats (it depends on n_hits only).  No rows, or a row with den = 0: N_ROWS = n_hits and NaN
 * in the other columns of every plane.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than out_field / kernel_ms, n <= 0, n_planes <= 0,
 * n_hits < 0.  The _sweep forms are in bmo_sweep_readout.h; there is no GaussianBeamlet form.
 *
 * bmo_result_psf_rows: the device pointer, the row count and (optional) the device ordinal of the rows of PSFDetector slot `detector` still
 * resident in `res`, to hand to the two calls above (hits_on_device != 0).  It is bmo_result_device_hits with the refusals of the _sweep
 * read-outs: BMO_ERR_INVALID for a null pointer, a slot out of range or not a PSFDetector's, or a sweep result; BMO_ERR_UNSUPPORTED for a
 * GaussianBeamlet result (three rows per beamlet).                                                                                      */
enum bmo_focus_stat {
    BMO_FOCUS_STAT_N_ROWS = 0,
    BMO_FOCUS_STAT_S = 1,
    BMO_FOCUS_STAT_CX = 2,
    BMO_FOCUS_STAT_CZ = 3,
    BMO_FOCUS_STAT_X_MIN = 4,
    BMO_FOCUS_STAT_X_MAX = 5,
    BMO_FOCUS_STAT_Z_MIN = 6,
    BMO_FOCUS_STAT_Z_MAX = 7,
    BMO_FOCUS_STAT_HWX = 8,
    BMO_FOCUS_STAT_HWZ = 9,
    BMO_FOCUS_STAT_RMS_R = 10,
    BMO_FOCUS_STAT_MAX_R = 11
};
#define BMO_FOCUS_STAT_N 12
int bmo_psf_through_focus(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                          const double e2[3], const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n,
                          int32_t device, double* out_intensity, double* out_field, double* kernel_ms);
int bmo_psf_focus_stats(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                        const double e2[3], const double axis[3], const double* offsets, int32_t n_planes, int32_t device, double* stats,
                        double* kernel_ms);
int bmo_result_psf_rows(bmo_trace_result* res, int32_t detector, const double** data, int64_t* count, int32_t* device);

/* ------------------------------------------------------------------------------------------------
 * MTF read-out: the transfer function of a PSFDetector's rows on a stack of planes, computed on the device from the rows where they lie.
 * Frequencies f = (fx, fz) are in cycles per metre in the detector's local (x, z) frame.  One sign and unit convention for both entries:
 *   T(f) = sum w * cis(-2 pi (fx * x + fz * z)),      MTF(f) = |T(f)| / T(0)
 * w the weight at the point (x, z): a row's proj at its intersection with the plane (geometric), or the intensity of an image sample
 * (diffraction).  freqs: [n_freqs][2], host.  otf: [n_planes][n_freqs][2] as (re, im); mtf: [n_planes][n_freqs]; sums: [n_planes], T(0).
 * Everything is FP64, each expression evaluated left to right as written, without contraction.  sincospi(t) = (sin(pi t), cos(pi t)) keeps
 * the rounding of 2 pi out of the argument.
 *
 * bmo_psf_geo_otf: hits, origin, e1, e2, axis, offsets, n_planes, device, kernel_ms as for bmo_psf_focus_stats.  centers: NULL or
 * [n_planes][2], (cx_m, cz_m), the point of plane m the phase is counted from ((0, 0) when NULL; the MTF does not depend on it).  Per row
 * and plane m:
 *   den, o_m, s, q, x, z: exactly the expressions of bmo_psf_focus_stats
 *   ax = x - cx_m,   az = z - cz_m
 *   a = fx * ax + fz * az,   (sn, cs) = sincospi(-2.0 * a)
 *   re += proj * cs,   im += proj * sn
 *   S = sum proj (equal to BMO_FOCUS_STAT_S bit for bit),   sums[m] = S,   mtf = sqrt(re * re + im * im) / S
 * The sums of (re, im) run over the rows of a split in row order and the splits (those of bmo_spot_stats) are folded in split order: a
 * fixed order that depends on n_hits only.  So the value at (plane, frequency) does not depend on which other planes or frequencies the
 * call asks for, and resident rows equal host rows, both bit for bit.  No rows: zeros, and NaN in mtf.  A row with den = 0 (or a NaN proj):
 * NaN everywhere.  BMO_ERR_LIMIT if the partial sums (16 bytes per split, plane and frequency; at most 2 048 splits) would pass 4 GiB: ask
 * for the planes or frequencies in several calls.
 *
 * bmo_psf_otf: hits .. displacements, n_planes, xs, zs, n, device as for bmo_psf_through_focus.  The images I_m are those of
 * bmo_psf_through_focus for the same arguments bit for bit (the same kernels and plan) and stay on the device; out_intensity: optional,
 * host, [n_planes][n*n].  The sample (i, j) of plane m has the local coordinates (xs[i], zs[j]) of its own displaced grid.  Per plane and
 * frequency:
 *   (sx_i, cx_i) = sincospi(-2.0 * (fx * xs[i])),   (sz_j, cz_j) = sincospi(-2.0 * (fz * zs[j]))
 *   row j:  r_re = sum_i I(i,j) * cx_i,   r_im = sum_i I(i,j) * sx_i                                                       (i ascending)
 *   T_re = sum_j (r_re * cz_j - r_im * sz_j),   T_im = sum_j (r_re * sz_j + r_im * cz_j)                                 (j ascending)
 *   sums[m]: the same two loops with the factor (1, 0) in place of both cis;   mtf = sqrt(T_re * T_re + T_im * T_im) / sums[m]
 * n_hits = 0: zeros, and NaN in mtf.  An image samples the PSF at the pitch of xs and zs: a frequency beyond 1 / (2 pitch) aliases (the
 * Python layer refuses it), and the window must hold the PSF without its replicas (components.mtf_window).
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than centers, out_intensity, kernel_ms; n_planes <= 0,
 * n_freqs <= 0, n <= 0, n_hits < 0; a frequency that is not finite.  The _sweep forms are in bmo_sweep_readout.h; there is no
 * GaussianBeamlet form.  Resident rows of an ordinary result come through bmo_result_psf_rows.                                          */
int bmo_psf_geo_otf(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                    const double e2[3], const double axis[3], const double* offsets, const double* centers, int32_t n_planes,
                    const double* freqs, int32_t n_freqs, int32_t device, double* otf, double* mtf, double* sums, double* kernel_ms);
int bmo_psf_otf(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* freqs,
                int32_t n_freqs, int32_t device, double* otf, double* mtf, double* sums, double* out_intensity, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Encircled-energy read-out: the share of the light inside a circle (encircled energy) or a square (ensquared energy) of half-size R about
 * a centre, for a list of R, computed on the device from the rows where they lie.  Shared by the four entries:
 *   shape: 0 = circle, 1 = square.   radii: [n_radii], host, in any order, each finite and >= 0.
 *   (ax, az): a point's local coordinates less the centre.
 *   circle:  r2 = ax * ax + az * az,   inside iff r2 <= R * R       (R * R computed once in FP64; there is no square root)
 *   square:  inside iff fabs(ax) <= R && fabs(az) <= R
 * Everything is FP64, each expression evaluated left to right as written, without contraction.  The compares are plain: a NaN is outside
 * every radius, and the edge is closed.
 *
 * bmo_spot_ee: rows, n_rows, row_cols, rows_on_device, device, kernel_ms as for bmo_spot_image (x in column 0, z in column 1).
 *   ax = x - center[0],   az = z - center[1];   inside[k]: the number of rows inside radii[k]
 * Counts are integers: exact, whatever the order of the adds.  n_radii <= 4096, BMO_ERR_LIMIT beyond.
 *
 * bmo_spot_ee_sweep: the resident rows of Spotdetector slot `detector` of `res`, one curve per configuration (n_configs = 1 for an ordinary
 * result; it works on record_segments = 0 results).  centers: [n_configs][2]; inside: [n_configs][n_radii]; n_rows: [n_configs], the rows
 * of each configuration.  Configuration c equals bmo_spot_ee on its rows exactly.  It refuses what bmo_spot_stats_sweep refuses.
 *
 * bmo_psf_geo_ee: hits .. n_planes and centers as for bmo_psf_geo_otf (centers NULL: (0, 0)).  Per row and plane m:
 *   den, o_m, s, q, x, z: exactly the expressions of bmo_psf_focus_stats
 *   ax = x - cx_m,   az = z - cz_m
 *   energy[m][k] = sum of proj over the rows inside radii[k],   count[m][k] their number (count: optional, NULL skips it)
 *   sums[m] = S = sum proj (equal to BMO_FOCUS_STAT_S bit for bit),   ee[m][k] = energy[m][k] / S
 * The sum of a (plane, radius) pair runs over the rows of a split in row order, starts at +0.0, and a row outside adds nothing; the splits
 * (those of bmo_spot_stats) are folded in split order.  So a pair's value does not depend on the planes and radii asked for along with it,
 * and resident rows equal host rows, both bit for bit.  No rows: zeros, and NaN in ee.  A row with den = 0 (or a NaN proj): NaN in ee,
 * energy and sums; count is still the plain count.  BMO_ERR_LIMIT if the partial sums (16 bytes per split, plane and radius; at most 2 048
 * splits) would pass 4 GiB: ask for the planes or radii in several calls.
 *
 * bmo_psf_ee: hits .. displacements, n_planes, xs, zs, n, device as for bmo_psf_through_focus.  The images I_m are those of
 * bmo_psf_through_focus for the same arguments bit for bit (the same kernels and plan) and stay on the device; out_intensity: optional,
 * host, [n_planes][n*n].  centers: NULL or [n_planes][2].  Per plane, i ascending inside and j ascending outside:
 *   sums[m] = sum_j (sum_i I(i,j))
 *   centers NULL:  cx = (sum_j (sum_i I(i,j) * xs[i])) / sums[m],   cz = (sum_j ((sum_i I(i,j)) * zs[j])) / sums[m]     (the centroid)
 *   otherwise:     (cx, cz) = centers[m];     centers_out[m] = (cx, cz), always the centre used
 *   ax = xs[i] - cx,   az = zs[j] - cz
 *   energy[m][k] = sum_j (sum_i (inside ? I(i,j) : nothing)),   ee[m][k] = energy[m][k] / sums[m]
 * The curve is a ratio of pixel sums: it is normalised by the energy inside the sampled window, not by the energy of the whole PSF, so
 * the window must hold the PSF (components.mtf_window), and a radius whose circle or square leaves the window only reads 1 (the Python
 * layer refuses it).  n_hits = 0: zeros, NaN in ee, and NaN in centers_out where centers is NULL.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than centers (PSF entries), count, out_intensity,
 * kernel_ms; n_radii <= 0, n_planes <= 0, n <= 0, n_hits or n_rows < 0; shape outside 0..1; a radius that is negative or not finite; a
 * centre that is not finite; row_cols outside 2..9; a wrong slot or n_configs.  BMO_ERR_UNSUPPORTED: a GaussianBeamlet result.  The two PSF
 * entries have no _sweep form and no GaussianBeamlet form: resident rows come through bmo_result_psf_rows.                              */
int bmo_spot_ee(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, const double center[2], int32_t shape,
                const double* radii, int32_t n_radii, int32_t device, int64_t* inside, double* kernel_ms);
int bmo_spot_ee_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* centers, int32_t shape, const double* radii,
                      int32_t n_radii, int64_t* inside, int64_t* n_rows, double* kernel_ms);
int bmo_psf_geo_ee(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3],
                   const double e2[3], const double axis[3], const double* offsets, const double* centers, int32_t n_planes, int32_t shape,
                   const double* radii, int32_t n_radii, int32_t device, double* ee, double* energy, int64_t* count, double* sums,
                   double* kernel_ms);
int bmo_psf_ee(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
               const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* centers,
               int32_t shape, const double* radii, int32_t n_radii, int32_t device, double* ee, double* energy, double* sums,
               double* centers_out, double* out_intensity, double* kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Polychromatic read-out: the rows of a PSFDetector split by wavelength band on the device, and the incoherent, spectrally weighted sum of
 * the bands' through-focus stacks with its transform.  A PSF row carries its wave number k in column 8; every read-out above sums the rows
 * it is given coherently, as intensity(psf) does.  Light of different wavelengths does not interfere: the image of a solve that mixes
 * wavelengths is the weighted sum of the per-wavelength images.  No reference counterpart.
 *
 * Bands.  A row belongs to band b iff row[8] == k_b, a plain FP64 compare (-0 == +0; a NaN belongs to no band).  The engine writes
 * k = 2 * 3.141592653589793 / lambda per ray (bmo_lane.hpp), so rows of one wavelength share their k bit for bit.
 * bmo_psf_bands_create: hits, n_hits, hits_on_device, device as for bmo_psf_intensity.
 *   ks == NULL, the discovery form: the bands are the distinct k of the rows, ascending; n_ks is ignored.  Only rows with a NaN k are
 *     unmatched.  Counts are integers and the bands a set: the result does not depend on the order in which the device finds them.
 *   ks != NULL: exactly those n_ks bands in the caller's order.  A band without rows is legal and has count 0.  A row whose k is none of them,
 *     or is NaN, is dropped and counted in `unmatched`.
 *   The handle owns a device copy of the matched rows, [sum of counts][9], band-major; within a band the rows keep their original order
 *   (the partition is stable: no atomic decides a position).  It does not depend on the lifetime of the result or buffer it was built from.
 *   The defining property: band b equals, bit for bit and in order, the rows hits[hits[:, 8] == k_b].
 * bmo_psf_bands_info: the band count, the matched rows (sum of counts), the unmatched rows and the device ordinal; each pointer may be NULL.
 * bmo_psf_bands_get: the band's k, the device pointer to its first row and its count (each pointer may be NULL).  The pointer is made to be
 *   handed to every read-out above that takes hits_on_device != 0, on the handle's device: such a call reads the band exactly as it reads
 *   host rows hits[hits[:, 8] == k_b].
 * bmo_psf_bands_free: frees the rows and the handle (NULL: nothing).
 *
 * bmo_psf_poly_through_focus: origin .. n as for bmo_psf_through_focus; all bands share the pose, the displacements and the grid
 * (intensities add only at the same physical point).  coeffs: [n_bands], host.  FP64, no contraction, left to right as written:
 *   I_b = the stack bmo_psf_through_focus returns for band b's rows and the same arguments, bit for bit (the same kernels and plan, run on
 *         the band's range); a band without rows gives zeros
 *   acc = coeffs[0] * I_0;   acc = acc + coeffs[b] * I_b  for b = 1 .. n_bands - 1 in band order   (a multiply and an add, never fused)
 *   out_intensity[m][i + n*j] = acc:  host, [n_planes][n*n].   out_band_intensity: optional, host, [n_bands][n_planes][n*n], the I_b.
 * No bands: zeros.
 *
 * bmo_psf_poly_otf: the combined stack stays on the device and is transformed by the row and column passes of bmo_psf_otf (the same
 * kernels, expressions and order, `acc` in the place of I): freqs, otf, mtf, sums as there.  By linearity T(f) = sum_b coeffs[b] T_b(f) and
 * sums = sum_b coeffs[b] T_b(0).  out_intensity: optional, equal to bmo_psf_poly_through_focus's bit for bit.  No bands or no matched rows:
 * zeros, and NaN in mtf.
 *
 * BMO_ERR_INVALID (checked before a device is looked for): a null pointer other than ks, the optional outputs and kernel_ms; n_hits < 0;
 * ks given with n_ks <= 0, with a k that is not finite, or with two equal k; n, n_planes or n_freqs <= 0; a coefficient or a frequency that
 * is not finite; a band index out of range.  BMO_ERR_LIMIT: n_ks > BMO_PSF_MAX_BANDS, or the discovery form finds more distinct k than that.
 * There is no _sweep form and no GaussianBeamlet form: resident rows come through bmo_result_psf_rows and inherit its refusals.
 * kernel_ms: optional, HIP-event time of the launches.                                                                                  */
#define BMO_PSF_MAX_BANDS 64
typedef struct bmo_psf_bands bmo_psf_bands;
int bmo_psf_bands_create(const double* hits, int64_t n_hits, int32_t hits_on_device, int32_t device, const double* ks, int32_t n_ks,
                         bmo_psf_bands** out, double* kernel_ms);
int bmo_psf_bands_info(const bmo_psf_bands* b, int32_t* n_bands, int64_t* n_rows, int64_t* unmatched, int32_t* device);
int bmo_psf_bands_get(const bmo_psf_bands* b, int32_t band, double* k, const double** rows, int64_t* count);
int bmo_psf_bands_free(bmo_psf_bands* b);
int bmo_psf_poly_through_focus(const bmo_psf_bands* b, const double origin[3], const double e1[3], const double e2[3],
                               const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n,
                               const double* coeffs, double* out_intensity, double* out_band_intensity, double* kernel_ms);
int bmo_psf_poly_otf(const bmo_psf_bands* b, const double origin[3], const double e1[3], const double e2[3], const double* displacements,
                     int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* coeffs, const double* freqs,
                     int32_t n_freqs, double* otf, double* mtf, double* sums, double* out_intensity, double* kernel_ms);

#ifdef __cplusplus
}
#endif
/* the _sweep forms of bmo_psf_focus_stats, bmo_psf_through_focus, bmo_psf_geo_otf and bmo_psf_otf */
#include "bmo_sweep_readout.h"
#endif /* BMO_H */
