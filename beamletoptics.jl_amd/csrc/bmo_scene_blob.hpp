// bmo_scene_blob.hpp — the scene blob: its format and the host code that builds it from a bmo_scene_desc (include/bmo.h).
// No HIP runtime call and no global of the engine: bmo_engine.hip includes it for the format and the builder, and a host compiler
// compiles it as it stands (tests/emu/scene_check.cpp runs the builder under the sanitizers).  Errors come back as a BMO_ERR_* code and
// a text; the C entry points in bmo_engine.hip hand them to fail().
//   BlobHeader, view_of     the format: a header of counts, tolerances and 32-bit offsets, the kernels' SceneView of a blob
//   BlobRegion, lay_out_blob  the layout: ONE list of the regions behind the header, walked to assign offsets and walked to copy
//   bvh_build               the mesh BVH (binned SAH)
//   SceneImage              what a build leaves: blob, header, BVH statistics, bounding sphere; several configurations after a merge
//   build_scene_image       validate_shapes, validate_objects, header_of, build_bvhs, blob_regions + lay_out_blob, fill_blob,
//                           patch_shape_flags, bound_candidates
//   sweep_topology_diff, merge_sweep_images   the configurations of a sweep in one image under one header
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "bmo_lane.hpp"

#if defined(__HIPCC__)
#define BMO_BLOB_HD __host__ __device__ inline
#else
#define BMO_BLOB_HD inline
#endif

namespace {
using namespace bmo;

// ------------------------------------------------------------------ scene blob (LDS image)
struct BlobHeader {
    int32_t n_objects, n_shapes, n_children, n_tris, n_media, n_lambda, n_detectors, march_iters;
    double eps_srf, eps_ray, eps_ins, mt_keps, mt_leps, grad_h;
    uint32_t off_objects, off_shapes, off_children, off_tris, off_ntable, total;
    uint32_t has_splitter, off_coefs;
    uint32_t has_asphere, off_cands;
    int32_t n_cands, has_meniscus, pad[2];  // pad[0] is has_bvh() below, the one spelling in use; the member keeps the name and type
                                            // that every earlier revision of tests/emu/scene_check.cpp compiles against
    uint32_t off_bvh_nodes, off_bvh_faces;  // mesh BVHs (bmo_lane.hpp BvhNode; face ids, int32)
    uint32_t off_boxes, pad2;               // the shapes' bounding boxes (bmo_lane.hpp box_cull), six doubles per shape id
    BMO_BLOB_HD int32_t has_bvh() const { return pad[0]; }  // 1: some mesh has a BVH (the kernels of level 3)
    BMO_BLOB_HD int32_t& has_bvh() { return pad[0]; }
};
static_assert(sizeof(BlobHeader) == 152, "BlobHeader travels in the step kernels' arguments (StepParams::hdr): its layout is part of their builds");

// `h`: the blob's header; the kernels read it from their arguments (scalar loads the compiler may repeat instead of holding the
// values in registers — read from the LDS copy they would sit in vector registers for the whole kernel)
template <class CharPtr>
BMO_BLOB_HD SceneView view_of(CharPtr blob, const BlobHeader* h) {
    SceneView S;
    S.objects = (CObject*)(blob + h->off_objects);
    S.shapes = (CShape*)(blob + h->off_shapes);
    S.children = (CInt*)(blob + h->off_children);
    S.tris = (CDouble*)(blob + h->off_tris);
    S.n_table = (CDouble*)(blob + h->off_ntable);
    S.coefs = (CDouble*)(blob + h->off_coefs);
    S.cands = (const BMO_KONST Cand*)(blob + h->off_cands);
    S.boxes = (CDouble*)(blob + h->off_boxes);
    S.n_cands = h->n_cands;
    S.n_objects = h->n_objects;
    S.n_lambda = h->n_lambda;
    S.eps_srf = h->eps_srf;
    S.eps_ray = h->eps_ray;
    S.eps_ins = h->eps_ins;
    S.mt_keps = h->mt_keps;
    S.mt_leps = h->mt_leps;
    S.grad_h = h->grad_h;
    S.march_iters = h->march_iters;
    if (h->has_bvh()) {
        S.bvh_nodes = (const BMO_KONST BvhNode*)(blob + h->off_bvh_nodes);
        S.bvh_faces = (CInt*)(blob + h->off_bvh_faces);
    }
    return S;
}

// One region of the blob behind the header: the header field that holds its offset, its size, and what is copied there (nullptr:
// the region stays zero until a later phase fills it).  Regions start on 16-byte boundaries.
struct BlobRegion {
    uint32_t BlobHeader::*off;
    size_t bytes;
    const void* src;
};
// Assigns every region's offset and the total, in list order.  false: the blob would pass 4 GiB (the kernels address it with 32-bit offsets).
inline bool lay_out_blob(const std::vector<BlobRegion>& regions, BlobHeader& h) {
    auto al = [](uint64_t x) { return (x + 15) & ~(uint64_t)15; };
    uint64_t off = al(sizeof(BlobHeader));
    for (const BlobRegion& r : regions) {
        h.*r.off = (uint32_t)off;
        off = al(off + r.bytes);
        if (off > 0xffffffffull) return false;
    }
    h.total = (uint32_t)off;
    return true;
}

// ------------------------------------------------------------------ mesh BVH builder
// Binned SAH (16 bins per axis over the face boxes' centres, traversal and triangle test weighted alike); leaves of at most
// BVH_MAX_LEAF faces unless the faces cannot be told apart by their centres.  Below depth BVH_SAH_DEPTH every split is an object
// median, so no BVH is deeper than BVH_SAH_DEPTH + 31 < BMO_BVH_MAX_DEPTH (the traversal's stack).  Face boxes are inflated as
// bmo_lane.hpp BvhNode says (the culling argument of mesh_nearest_bvh).
constexpr int BVH_BINS = 16, BVH_MAX_LEAF = 8, BVH_SAH_DEPTH = 32;
static_assert(BVH_SAH_DEPTH + 31 <= BMO_BVH_MAX_DEPTH, "median splits below BVH_SAH_DEPTH must fit the traversal stack");
static_assert(sizeof(BvhNode) == 64, "BvhNode layout");
struct BvhStats {
    int32_t n_nodes = 0, depth = 0, max_leaf = 0;
};
struct Box3 {
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    void grow(const Box3& b) {
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], b.lo[a]), hi[a] = std::max(hi[a], b.hi[a]);
    }
    double area() const {
        const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
        return x < 0 ? 0.0 : 2 * (x * y + y * z + z * x);
    }
};
// Appends the BVH of the `nf` faces at `tri` (9 doubles each) to nodes / faces (absolute indices; face ids are 0-based in the mesh) and
// returns the index of its header node, or -1 (nothing appended) when the mesh cannot have one: a non-finite vertex, or kϵ not > 0.
inline int bvh_build(const double* tri, int nf, double keps, std::vector<BvhNode>& nodes, std::vector<int32_t>& faces, BvhStats& st) {
    if (!(keps > 0.0) || !std::isfinite(keps) || nf < 1) return -1;
    std::vector<Box3> fb((size_t)nf);
    std::vector<double> cen((size_t)nf * 3);
    double g = 0.0;  // max |E1| |E2|
    for (int f = 0; f < nf; ++f) {
        const double* v = tri + 9 * (size_t)f;
        double e1 = 0, e2 = 0, m = 0;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(v[a]) || !std::isfinite(v[3 + a]) || !std::isfinite(v[6 + a])) return -1;
            const double d1 = v[3 + a] - v[a], d2 = v[6 + a] - v[a];
            e1 += d1 * d1, e2 += d2 * d2;
            m = std::max(m, std::max(std::fabs(v[a]), std::max(std::fabs(v[3 + a]), std::fabs(v[6 + a]))));
        }
        e1 = std::sqrt(e1), e2 = std::sqrt(e2);
        g = std::max(g, e1 * e2);
        const double infl = 4 * keps * std::max(e1, e2) + 0x1p-46 * m;
        Box3& b = fb[(size_t)f];
        for (int a = 0; a < 3; ++a) {
            b.lo[a] = std::min(v[a], std::min(v[3 + a], v[6 + a])) - infl;
            b.hi[a] = std::max(v[a], std::max(v[3 + a], v[6 + a])) + infl;
            cen[3 * (size_t)f + a] = 0.5 * b.lo[a] + 0.5 * b.hi[a];
        }
    }
    std::vector<int32_t> idx((size_t)nf);
    for (int f = 0; f < nf; ++f) idx[(size_t)f] = f;
    const int32_t hdr = (int32_t)nodes.size();
    const int32_t face0 = (int32_t)faces.size();
    nodes.resize(nodes.size() + 2);  // header, root
    st = BvhStats{};
    // one node: its box, then a leaf or a split into two consecutive children
    auto build = [&](auto&& self, int32_t ni, int begin, int end, int depth) -> void {
        Box3 box, cb;
        for (int i = begin; i < end; ++i) {
            const int f = idx[(size_t)i];
            box.grow(fb[(size_t)f]);
            for (int a = 0; a < 3; ++a)
                cb.lo[a] = std::min(cb.lo[a], cen[3 * (size_t)f + a]), cb.hi[a] = std::max(cb.hi[a], cen[3 * (size_t)f + a]);
        }
        for (int a = 0; a < 3; ++a) nodes[(size_t)ni].lo[a] = box.lo[a], nodes[(size_t)ni].hi[a] = box.hi[a];
        st.depth = std::max(st.depth, depth);
        const int n = end - begin;
        int axis = 0;
        for (int a = 1; a < 3; ++a)
            if (cb.hi[a] - cb.lo[a] > cb.hi[axis] - cb.lo[axis]) axis = a;
        int mid = -1;
        if (n > 2 && depth < BVH_SAH_DEPTH) {
            double best = (double)n * box.area();  // leaf cost
            int best_axis = -1, best_bin = 0;
            for (int a = 0; a < 3; ++a) {
                const double ext = cb.hi[a] - cb.lo[a];
                if (!(ext > 0)) continue;
                Box3 bb[BVH_BINS];
                int cnt[BVH_BINS] = {};
                const double k = BVH_BINS / ext;
                for (int i = begin; i < end; ++i) {
                    const int f = idx[(size_t)i];
                    const int bin = std::min(BVH_BINS - 1, (int)((cen[3 * (size_t)f + a] - cb.lo[a]) * k));
                    cnt[bin] += 1;
                    bb[bin].grow(fb[(size_t)f]);
                }
                double right_area[BVH_BINS];
                int right_n[BVH_BINS];
                Box3 acc;
                int an = 0;
                for (int b = BVH_BINS - 1; b > 0; --b) {
                    acc.grow(bb[b]);
                    an += cnt[b];
                    right_area[b] = acc.area(), right_n[b] = an;
                }
                acc = Box3{};
                an = 0;
                for (int b = 0; b < BVH_BINS - 1; ++b) {  // split between bin b and b + 1
                    acc.grow(bb[b]);
                    an += cnt[b];
                    if (an == 0 || right_n[b + 1] == 0) continue;
                    const double c = box.area() + acc.area() * an + right_area[b + 1] * right_n[b + 1];
                    if (c < best) best = c, best_axis = a, best_bin = b;
                }
            }
            if (best_axis >= 0) {
                const double k = BVH_BINS / (cb.hi[best_axis] - cb.lo[best_axis]);
                auto it = std::partition(idx.begin() + begin, idx.begin() + end, [&](int f) {
                    return std::min(BVH_BINS - 1, (int)((cen[3 * (size_t)f + best_axis] - cb.lo[best_axis]) * k)) <= best_bin;
                });
                mid = (int)(it - idx.begin());
                axis = best_axis;
            }
        }
        if (mid < 0 && (n > BVH_MAX_LEAF || (depth >= BVH_SAH_DEPTH && n > 2))) {  // object median (also for faces with equal centres)
            mid = begin + n / 2;
            std::nth_element(idx.begin() + begin, idx.begin() + mid, idx.begin() + end,
                             [&](int x, int y) { return cen[3 * (size_t)x + axis] < cen[3 * (size_t)y + axis]; });
        }
        if (mid <= begin || mid >= end) {  // leaf
            BvhNode& nd = nodes[(size_t)ni];
            nd.first = face0 + begin, nd.count = n, nd.axis = 0;
            st.max_leaf = std::max(st.max_leaf, n);
            return;
        }
        const int32_t c = (int32_t)nodes.size();
        nodes.resize(nodes.size() + 2);
        nodes[(size_t)ni].first = c, nodes[(size_t)ni].count = 0, nodes[(size_t)ni].axis = axis;
        self(self, c, begin, mid, depth + 1);
        self(self, c + 1, mid, end, depth + 1);
    };
    build(build, hdr + 1, 0, nf, 1);
    faces.insert(faces.end(), idx.begin(), idx.end());
    BvhNode& H = nodes[(size_t)hdr];
    const BvhNode& R = nodes[(size_t)hdr + 1];
    double d2 = 0;
    for (int a = 0; a < 3; ++a) {
        H.lo[a] = 0.5 * R.lo[a] + 0.5 * R.hi[a];
        d2 += (R.hi[a] - R.lo[a]) * (R.hi[a] - R.lo[a]);
    }
    H.hi[0] = 0.5 * std::sqrt(d2) * (1 + 0x1p-40);  // (rounded up: D must bound |pos - V|)
    H.hi[1] = 0x1p-46 * g / keps;
    H.hi[2] = 0;
    H.first = hdr + 1, H.count = 0, H.axis = 0;
    st.n_nodes = (int32_t)nodes.size() - hdr - 1;
    return hdr;
}

// ------------------------------------------------------------------ the scene builder
struct SceneImage {
    std::vector<char> blob;
    BlobHeader hdr;
    std::vector<size_t> region_bytes;  // the size of every region of blob_regions' list, in its order (what lay_out_blob gave `hdr` its offsets from)
    std::vector<BvhStats> bvh;  // per shape (n_nodes = 0: no BVH)
    double bound[4] = {0, 0, 0, -1};  // a sphere around the bounding spheres of all candidates (centre, radius; radius < 0: none) — root_chord_kernel
    // merge_sweep_images: n_configs blobs of `stride` bytes each, back to back in `blob`, all described by `hdr` (0: an ordinary scene)
    int32_t n_configs = 0;
    uint64_t stride = 0;
};
// the mesh BVHs of a description: node and face tables of all of them, and every shape's header node (-1: none)
struct SceneBvhs {
    std::vector<BvhNode> nodes;
    std::vector<int32_t> faces, hdr_of;
};

inline int refuse(std::string& err, int code, const char* msg) {
    err = msg;
    return code;
}

inline int validate_shapes(const bmo_scene_desc* d, std::string& err) {
    for (int i = 0; i < d->n_shapes; ++i) {
        const bmo_shape& s = d->shapes[i];
        if (s.kind < 0 || s.kind >= BMO_SHAPE_KIND_COUNT) return refuse(err, BMO_ERR_UNSUPPORTED, "unknown shape kind");
        if (s.kind == BMO_SHAPE_UNION || s.kind == BMO_SHAPE_MENISCUS) {
            if (s.child_begin < 0 || s.child_begin + s.child_count > d->n_children || s.child_count < 1)
                return refuse(err, BMO_ERR_INVALID, "child range out of bounds");
            if (s.kind == BMO_SHAPE_MENISCUS && s.child_count != 3) return refuse(err, BMO_ERR_INVALID, "meniscus needs 3 children");
            for (int c = 0; c < s.child_count; ++c) {
                int ch = d->children[s.child_begin + c];
                if (ch < 0 || ch >= d->n_shapes) return refuse(err, BMO_ERR_INVALID, "child id out of bounds");
                int ck = d->shapes[ch].kind;
                if (ck == BMO_SHAPE_UNION || ck == BMO_SHAPE_MESH) return refuse(err, BMO_ERR_INVALID, "nested union / mesh child");
                if (s.kind == BMO_SHAPE_MENISCUS && ck == BMO_SHAPE_MENISCUS) return refuse(err, BMO_ERR_INVALID, "nested meniscus");
            }
        }
        if ((s.kind == BMO_SHAPE_ASPH_CONVEX || s.kind == BMO_SHAPE_ASPH_CONCAVE || s.kind == BMO_SHAPE_ACYL_CONVEX || s.kind == BMO_SHAPE_ACYL_CONCAVE) &&
            (s.child_begin < 0 || s.child_count < 0 || s.child_begin + s.child_count > d->n_coefs))
            return refuse(err, BMO_ERR_INVALID, "aspheric coefficient range out of bounds");
        if (s.kind == BMO_SHAPE_MESH && (s.tri_begin < 0 || s.tri_begin + s.tri_count > d->n_tris))
            return refuse(err, BMO_ERR_INVALID, "triangle range out of bounds");
    }
    return BMO_OK;
}

inline int validate_objects(const bmo_scene_desc* d, std::string& err) {
    for (int i = 0; i < d->n_objects; ++i) {
        const bmo_object& o = d->objects[i];
        if (o.kind < 0 || o.kind >= BMO_OBJ_KIND_COUNT) return refuse(err, BMO_ERR_UNSUPPORTED, "unknown object kind");
        int np = (o.kind == BMO_OBJ_DOUBLET || o.kind == BMO_OBJ_PLATE_BS) ? 2 : (o.kind == BMO_OBJ_CUBE_BS ? 3 : 1);
        for (int k = 0; k < np; ++k)
            if (o.shape[k] < 0 || o.shape[k] >= d->n_shapes) return refuse(err, BMO_ERR_INVALID, "object shape id out of bounds");
        for (int k = 0; k < 2; ++k)
            if (o.medium[k] >= d->n_media) return refuse(err, BMO_ERR_INVALID, "medium id out of bounds");
        if ((o.kind == BMO_OBJ_REFRACTIVE || o.kind == BMO_OBJ_DOUBLET || o.kind == BMO_OBJ_PLATE_BS || o.kind == BMO_OBJ_CUBE_BS) && o.medium[0] < 0)
            return refuse(err, BMO_ERR_INVALID, "refractive object without medium");
        if ((o.kind == BMO_OBJ_DOUBLET || o.kind == BMO_OBJ_CUBE_BS) && o.medium[1] < 0) return refuse(err, BMO_ERR_INVALID, "missing second medium");
        if ((o.kind == BMO_OBJ_SPOTDETECTOR || o.kind == BMO_OBJ_PSFDETECTOR || o.kind == BMO_OBJ_PHOTODETECTOR) &&
            (o.detector < 0 || o.detector >= d->n_detectors))
            return refuse(err, BMO_ERR_INVALID, "detector slot out of bounds");
    }
    return BMO_OK;
}

// counts, tolerances and the has_* flags of a validated description (the offsets: lay_out_blob; has_bvh: build_scene_image)
inline BlobHeader header_of(const bmo_scene_desc* d) {
    BlobHeader h{};
    h.n_objects = d->n_objects;
    h.n_shapes = d->n_shapes;
    h.n_children = d->n_children;
    h.n_tris = d->n_tris;
    h.n_media = d->n_media;
    h.n_lambda = d->n_lambda;
    h.n_detectors = d->n_detectors;
    h.march_iters = d->march_iters;
    h.eps_srf = d->eps_srf;
    h.eps_ray = d->eps_ray;
    h.eps_ins = d->eps_ins;
    h.mt_keps = d->mt_keps;
    h.mt_leps = d->mt_leps;
    h.grad_h = d->grad_h;
    for (int i = 0; i < d->n_objects; ++i) {
        const int k = d->objects[i].kind;
        if (k == BMO_OBJ_THIN_BS || k == BMO_OBJ_PLATE_BS || k == BMO_OBJ_CUBE_BS) h.has_splitter = 1;
    }
    for (int i = 0; i < d->n_shapes; ++i) {
        const int k = d->shapes[i].kind;
        if (k >= BMO_SHAPE_ASPH_CONVEX && k <= BMO_SHAPE_ACYL_CONCAVE) h.has_asphere = 1;  // extended shapes
        if (k == BMO_SHAPE_MENISCUS) h.has_meniscus = 1;
    }
    h.n_cands = fill_candidates(d->objects, d->n_objects, d->shapes, nullptr);
    return h;
}

// mesh BVHs (bvh_build above): every MESH of BMO_MESH_BVH_MIN_FACES faces or more unless its input flags say BMO_SHAPE_FLAG_NO_BVH
inline int build_bvhs(const bmo_scene_desc* d, SceneBvhs& B, std::vector<BvhStats>& stats, std::string& err) {
    B.hdr_of.assign((size_t)d->n_shapes, -1);
    stats.assign((size_t)d->n_shapes, BvhStats{});
    for (int i = 0; i < d->n_shapes; ++i) {
        const bmo_shape& s = d->shapes[i];
        if (s.kind != BMO_SHAPE_MESH || s.tri_count < BMO_MESH_BVH_MIN_FACES || (s.flags & BMO_SHAPE_FLAG_NO_BVH)) continue;
        B.hdr_of[(size_t)i] = bvh_build(d->tris + 9 * (size_t)s.tri_begin, s.tri_count, d->mt_keps, B.nodes, B.faces, stats[(size_t)i]);
        if (B.hdr_of[(size_t)i] >= 0 && stats[(size_t)i].depth > BMO_BVH_MAX_DEPTH) return refuse(err, BMO_ERR_INTERNAL, "mesh BVH deeper than the traversal stack");
    }
    return BMO_OK;
}

// THE list of the blob's regions, in blob order: a new table is added here and to BlobHeader / view_of, nowhere else.
inline std::vector<BlobRegion> blob_regions(const bmo_scene_desc* d, const BlobHeader& h, const SceneBvhs& B) {
    using H = BlobHeader;
    return {
        {&H::off_objects, sizeof(bmo_object) * (size_t)d->n_objects, d->objects},
        {&H::off_shapes, sizeof(bmo_shape) * (size_t)d->n_shapes, d->shapes},
        {&H::off_children, 4 * (size_t)d->n_children, d->children},
        {&H::off_tris, 72 * (size_t)d->n_tris, d->tris},
        {&H::off_ntable, 8 * (size_t)std::max(1, d->n_media) * (size_t)d->n_lambda, d->n_media ? d->n_table : nullptr},
        {&H::off_coefs, 8 * (size_t)std::max(1, d->n_coefs), d->n_coefs > 0 ? d->coefs : nullptr},
        // filled by fill_candidates (+ 3 zero entries: the collection of tracing_step reads four per trip)
        {&H::off_cands, sizeof(Cand) * (size_t)(std::max(1, h.n_cands) + 3), nullptr},
        {&H::off_bvh_nodes, sizeof(BvhNode) * B.nodes.size(), B.nodes.data()},
        {&H::off_bvh_faces, 4 * B.faces.size(), B.faces.data()},
        // filled by fill_blob from the shape table (shape_box)
        {&H::off_boxes, 8 * (size_t)BMO_BOX_DOUBLES * (size_t)std::max(1, d->n_shapes), nullptr},
    };
}

// the header, every region that has a source, the candidate table (trace_all's flat slot list), the shapes' boxes
inline void fill_blob(SceneImage& img, const bmo_scene_desc* d, const std::vector<BlobRegion>& regions) {
    const BlobHeader& h = img.hdr;
    img.blob.assign(h.total, 0);
    std::memcpy(img.blob.data(), &h, sizeof h);
    img.region_bytes.clear();
    for (const BlobRegion& r : regions) {
        if (r.src && r.bytes) std::memcpy(img.blob.data() + h.*r.off, r.src, r.bytes);
        img.region_bytes.push_back(r.bytes);
    }
    fill_candidates(d->objects, d->n_objects, d->shapes, reinterpret_cast<Cand*>(img.blob.data() + h.off_cands));
    for (int i = 0; i < d->n_shapes; ++i) {
        const ShapeBox b = shape_box(d->shapes, d->children, i);
        char* at = img.blob.data() + h.off_boxes + 8 * (size_t)BMO_BOX_DOUBLES * (size_t)i;
        std::memcpy(at, b.lo, sizeof b.lo);
        std::memcpy(at + sizeof b.lo, b.hi, sizeof b.hi);
    }
}

// The blob's shape flags are the builder's, whatever the description's say.  Unions whose children sit back to back in the shape
// table: no children[] look-up on the device.  Meshes with a BVH: the flag, and child_begin (unused by meshes) -> the BVH's header node.
inline void patch_shape_flags(SceneImage& img, const bmo_scene_desc* d, const SceneBvhs& B) {
    bmo_shape* shapes = reinterpret_cast<bmo_shape*>(img.blob.data() + img.hdr.off_shapes);
    for (int i = 0; i < d->n_shapes; ++i) {
        bmo_shape* sh = shapes + i;
        sh->flags &= ~(BMO_SHAPE_FLAG_CONSECUTIVE | BMO_SHAPE_FLAG_BVH);
        if (B.hdr_of[(size_t)i] >= 0) {
            sh->flags |= BMO_SHAPE_FLAG_BVH;
            sh->child_begin = B.hdr_of[(size_t)i];
        }
        if (sh->kind != BMO_SHAPE_UNION || sh->child_count <= 0) continue;
        bool consecutive = true;
        for (int c = 1; c < sh->child_count; ++c)
            if (d->children[sh->child_begin + c] != d->children[sh->child_begin] + c) consecutive = false;
        if (consecutive) {
            sh->flags |= BMO_SHAPE_FLAG_CONSECUTIVE;
            sh->tri_begin = d->children[sh->child_begin];
        }
    }
}

// the scene's bounding sphere: centre of the box around the candidates' spheres, radius to the farthest of them
inline void bound_candidates(SceneImage& img) {
    const Cand* cd = reinterpret_cast<const Cand*>(img.blob.data() + img.hdr.off_cands);
    const int n = img.hdr.n_cands;
    auto usable = [&](int i) { return cd[i].R >= 0.0 && std::isfinite(cd[i].R); };
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    int nb = 0;
    for (int i = 0; i < n; ++i) {
        if (!usable(i)) continue;
        const double c[3] = {cd[i].cx, cd[i].cy, cd[i].cz};
        for (int a = 0; a < 3; ++a) lo[a] = std::min(lo[a], c[a] - cd[i].R), hi[a] = std::max(hi[a], c[a] + cd[i].R);
        ++nb;
    }
    if (!nb) return;
    double R = 0.0;
    for (int a = 0; a < 3; ++a) img.bound[a] = 0.5 * (lo[a] + hi[a]);
    for (int i = 0; i < n; ++i) {
        if (!usable(i)) continue;
        const double dx = cd[i].cx - img.bound[0], dy = cd[i].cy - img.bound[1], dz = cd[i].cz - img.bound[2];
        R = std::max(R, std::sqrt(dx * dx + dy * dy + dz * dz) + cd[i].R);
    }
    img.bound[3] = R;
}

// bmo_scene_create without the handle: `img` is a fresh SceneImage (or one derived from it)
inline int build_scene_image(const bmo_scene_desc* d, SceneImage& img, std::string& err) {
    if (d->abi_version != BMO_ABI_VERSION) return refuse(err, BMO_ERR_INVALID, "abi version mismatch");
    if (d->n_objects < 0 || d->n_shapes < 0 || d->n_lambda < 1) return refuse(err, BMO_ERR_INVALID, "bad counts");
    if (int rc = validate_shapes(d, err)) return rc;
    if (int rc = validate_objects(d, err)) return rc;
    const char* too_big = "scene blob larger than 4 GiB (32-bit table offsets): fewer triangles or smaller tables";
    img.hdr = header_of(d);
    SceneBvhs B;
    // the list with empty BVH tables is a lower bound: a description that is too large is refused here, before any triangle is read
    if (!lay_out_blob(blob_regions(d, img.hdr, B), img.hdr)) return refuse(err, BMO_ERR_INVALID, too_big);
    if (int rc = build_bvhs(d, B, img.bvh, err)) return rc;
    img.hdr.has_bvh() = B.nodes.empty() ? 0 : 1;
    const std::vector<BlobRegion> regions = blob_regions(d, img.hdr, B);  // (its sources live as long as `d` and `B`: this function)
    if (!lay_out_blob(regions, img.hdr)) return refuse(err, BMO_ERR_INVALID, too_big);
    fill_blob(img, d, regions);
    patch_shape_flags(img, d, B);
    bound_candidates(img);
    return BMO_OK;
}

// ------------------------------------------------------------------ sweeps: several configurations in one image
// Topology of configuration `d` against configuration 0 (merge_sweep_images): "" when they agree, else the first field that differs.
inline std::string sweep_topology_diff(const bmo_scene_desc* a, const bmo_scene_desc* d) {
    auto ne = [](const void* x, const void* y, size_t n) { return std::memcmp(x, y, n) != 0; };
#define BMO_CMP(f) \
    if (a->f != d->f) return #f;
    BMO_CMP(abi_version) BMO_CMP(n_objects) BMO_CMP(n_shapes) BMO_CMP(n_children) BMO_CMP(n_tris) BMO_CMP(n_media) BMO_CMP(n_lambda) BMO_CMP(n_detectors)
    BMO_CMP(n_coefs) BMO_CMP(march_iters)
#undef BMO_CMP
    if (a->n_lambda > 0 && ne(a->lambdas, d->lambdas, 8 * (size_t)a->n_lambda)) return "lambdas";
    const double ka[6] = {a->eps_srf, a->eps_ray, a->eps_ins, a->mt_keps, a->mt_leps, a->grad_h}, kd[6] = {d->eps_srf, d->eps_ray, d->eps_ins, d->mt_keps, d->mt_leps, d->grad_h};
    const char* kn[6] = {"eps_srf", "eps_ray", "eps_ins", "mt_keps", "mt_leps", "grad_h"};
    for (int q = 0; q < 6; ++q)
        if (ne(&ka[q], &kd[q], 8)) return kn[q];
    for (int i = 0; i < a->n_objects; ++i) {
        const bmo_object &x = a->objects[i], &y = d->objects[i];
        const std::string at = "objects[" + std::to_string(i) + "].";
        if (x.kind != y.kind) return at + "kind";
        if (ne(x.shape, y.shape, sizeof x.shape)) return at + "shape";
        if (ne(x.medium, y.medium, sizeof x.medium)) return at + "medium";
        if (x.detector != y.detector) return at + "detector";
    }
    for (int i = 0; i < a->n_shapes; ++i) {
        const bmo_shape &x = a->shapes[i], &y = d->shapes[i];
        const std::string at = "shapes[" + std::to_string(i) + "].";
        if (x.kind != y.kind) return at + "kind";
        if (x.child_begin != y.child_begin) return at + "child_begin";
        if (x.child_count != y.child_count) return at + "child_count";
        if (x.tri_begin != y.tri_begin) return at + "tri_begin";
        if (x.tri_count != y.tri_count) return at + "tri_count";
        if (x.flags != y.flags) return at + "flags";
    }
    if (a->n_children > 0 && ne(a->children, d->children, 4 * (size_t)a->n_children)) return "children";
    return "";
}

// the images of the configurations, each built on its own from a description of configuration 0's topology
inline int build_sweep_configs(const bmo_scene_desc* descs, int32_t n_configs, std::vector<SceneImage>& cfg, std::string& err) {
    cfg.resize((size_t)n_configs);
    for (int32_t c = 0; c < n_configs; ++c) {
        const std::string at = "bmo_scene_create_sweep: configuration " + std::to_string(c);
        if (c > 0) {
            const std::string diff = sweep_topology_diff(&descs[0], &descs[c]);
            if (!diff.empty()) {
                err = at + " differs from configuration 0 in " + diff + " (a sweep changes numbers, not topology)";
                return BMO_ERR_INVALID;
            }
        }
        std::string why;
        if (const int rc = build_scene_image(&descs[c], cfg[(size_t)c], why)) {
            err = at + ": " + why;
            return rc;
        }
    }
    return BMO_OK;
}

// bmo_scene_create_sweep without the handle.  Every region but the mesh BVHs has the same size in every configuration; each region is
// sized to the largest one, so that every configuration has the same offsets and ONE header describes all of them.  A configuration's
// regions are copied one by one from where its own header has them (shapes keep their own BVH node indices).
inline int merge_sweep_images(const bmo_scene_desc* descs, int32_t n_configs, SceneImage& img, std::string& err) {
    std::vector<SceneImage> cfg;
    if (int rc = build_sweep_configs(descs, n_configs, cfg, err)) return rc;
    const BlobHeader& h0 = cfg[0].hdr;
    // the list of configuration 0 without sources (nothing is copied from a description here), every region sized to the largest
    std::vector<BlobRegion> regions = blob_regions(&descs[0], h0, SceneBvhs{});
    for (size_t r = 0; r < regions.size(); ++r) regions[r] = BlobRegion{regions[r].off, cfg[0].region_bytes[r], nullptr};
    for (int32_t c = 0; c < n_configs; ++c) {
        const BlobHeader& h = cfg[(size_t)c].hdr;
        if (h.n_cands != h0.n_cands || h.has_bvh() != h0.has_bvh() || h.off_bvh_nodes != h0.off_bvh_nodes || h.has_splitter != h0.has_splitter) {
            err = "bmo_scene_create_sweep: configuration " + std::to_string(c) + " differs from configuration 0 in its candidate table or BVHs";
            return BMO_ERR_INVALID;
        }
        for (size_t r = 0; r < regions.size(); ++r) regions[r].bytes = std::max(regions[r].bytes, cfg[(size_t)c].region_bytes[r]);
    }
    BlobHeader H = h0;
    if (!lay_out_blob(regions, H)) return refuse(err, BMO_ERR_INVALID, "bmo_scene_create_sweep: scene blob larger than 4 GiB (32-bit table offsets)");
    const uint64_t stride = ((uint64_t)H.total + 255) & ~(uint64_t)255;  // configurations start on 256-byte boundaries (scalar cache lines)
    try {
        img.blob.assign((size_t)(stride * (uint64_t)n_configs), 0);
    } catch (const std::bad_alloc&) {
        return refuse(err, BMO_ERR_OOM, "bmo_scene_create_sweep: host allocation of the configurations' blobs");
    }
    for (int32_t c = 0; c < n_configs; ++c) {
        const SceneImage& one = cfg[(size_t)c];
        char* dst = img.blob.data() + stride * (uint64_t)c;
        std::memcpy(dst, &H, sizeof H);
        for (size_t r = 0; r < regions.size(); ++r) {
            const size_t bytes = one.region_bytes[r];
            if (bytes) std::memcpy(dst + H.*regions[r].off, one.blob.data() + one.hdr.*regions[r].off, bytes);
        }
    }
    img.hdr = H;
    for (const BlobRegion& r : regions) img.region_bytes.push_back(r.bytes);
    img.bvh = cfg[0].bvh;
    std::memcpy(img.bound, cfg[0].bound, sizeof img.bound);
    img.n_configs = n_configs;
    img.stride = stride;
    return BMO_OK;
}

}  // namespace
