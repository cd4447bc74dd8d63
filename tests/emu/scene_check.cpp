// TEST-ONLY stand-alone program: the scene builder of bmo_scene_blob.hpp (validation, mesh BVHs, blob layout, sweep merge) under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/emu/Makefile; run by tests/test_scene_build_host.py).  It reads no file: every
// input comes from a fixed seed, and every array of a description is allocated at exactly its stated length, so that a read past a table
// is a heap overflow the sanitizer sees.  Exit status 0: every check held; the first failed check prints itself and exits 1.
// It prints an FNV-1a hash of every blob it built (two builds of the same builder print the same lines).
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "../../beamletoptics.jl_amd/csrc/bmo_scene_blob.hpp"

namespace {

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                               \
            std::printf("\n");                                      \
            std::exit(1);                                           \
        }                                                           \
    } while (0)

struct Rng {  // (the generator of bmo_selftest)
    unsigned long long s;
    double operator()() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1p-53;
    }
    double in(double lo, double hi) { return lo + (hi - lo) * (*this)(); }
};

template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // a heap block of exactly v.size() elements (none: no block at all)
    if (v.empty()) return nullptr;
    std::unique_ptr<T[]> p(new T[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// A description under construction (vectors) and the one handed to the builder (exact-length blocks).
struct Desc {
    std::vector<bmo_object> objects;
    std::vector<bmo_shape> shapes;
    std::vector<int32_t> children;
    std::vector<double> tris, n_table, lambdas{1.064e-6, 532e-9}, coefs;
    int n_media = 1, n_detectors = 1;
    double mt_keps = 1e-9;
    std::function<void(bmo_scene_desc&)> tweak;  // the last word on the counts (refusals)
    std::unique_ptr<bmo_object[]> e_objects;
    std::unique_ptr<bmo_shape[]> e_shapes;
    std::unique_ptr<int32_t[]> e_children;
    std::unique_ptr<double[]> e_tris, e_n_table, e_lambdas, e_coefs;
    bmo_scene_desc d;
    const bmo_scene_desc* finish() {
        n_table.assign((size_t)std::max(0, n_media) * lambdas.size(), 1.5);
        e_objects = exact(objects), e_shapes = exact(shapes), e_children = exact(children), e_tris = exact(tris);
        e_n_table = exact(n_table), e_lambdas = exact(lambdas), e_coefs = exact(coefs);
        d = bmo_scene_desc{};
        d.abi_version = BMO_ABI_VERSION;
        d.n_objects = (int32_t)objects.size(), d.n_shapes = (int32_t)shapes.size(), d.n_children = (int32_t)children.size();
        d.n_tris = (int32_t)(tris.size() / 9), d.n_media = n_media, d.n_lambda = (int32_t)lambdas.size(), d.n_detectors = n_detectors;
        d.n_coefs = (int32_t)coefs.size();
        d.objects = e_objects.get(), d.shapes = e_shapes.get(), d.children = e_children.get(), d.tris = e_tris.get();
        d.n_table = e_n_table.get(), d.lambdas = e_lambdas.get(), d.coefs = e_coefs.get();
        d.eps_srf = 1e-9, d.eps_ray = 1e-10, d.eps_ins = 1.0, d.mt_keps = mt_keps, d.mt_leps = 1e-9, d.grad_h = 1e-8, d.march_iters = 1000;
        if (tweak) tweak(d);
        return &d;
    }
};

bmo_shape shape(int kind, double x, double y, double z, double r) {
    bmo_shape s{};
    s.kind = kind;
    s.pos[0] = x, s.pos[1] = y, s.pos[2] = z;
    for (int a = 0; a < 3; ++a) s.dir[4 * a] = s.tdir[4 * a] = 1.0;
    s.p[0] = r, s.p[1] = r, s.p[2] = 0.1 * r, s.p[3] = r;
    s.bs_center[0] = x, s.bs_center[1] = y, s.bs_center[2] = z;
    s.bs_radius = 2 * r;
    return s;
}
bmo_shape group(int kind, int child_begin, int child_count, double y) {
    bmo_shape s = shape(kind, 0, y, 0, 0.02);
    s.child_begin = child_begin, s.child_count = child_count;
    return s;
}
bmo_object object(int kind, int s0, int s1 = -1, int s2 = -1, int m0 = -1, int m1 = -1, int det = -1) {
    bmo_object o{};
    o.kind = kind;
    o.shape[0] = s0, o.shape[1] = s1, o.shape[2] = s2;
    o.medium[0] = m0, o.medium[1] = m1;
    o.detector = det;
    o.reflectance = o.transmittance = 0.7071;
    return o;
}

// Two lenses and a detector: shape 3 is a union of the consecutive shapes 0, 1, 2; shape 6 one of shapes 5, 4 (not consecutive).
Desc two_lens_scene() {
    Desc D;
    D.shapes = {shape(BMO_SHAPE_CONVEX, 0, 0, 0, 0.01), shape(BMO_SHAPE_CYLINDER, 0, 0.002, 0, 0.01), shape(BMO_SHAPE_CONCAVE, 0, 0.004, 0, 0.01),
                group(BMO_SHAPE_UNION, 0, 3, 0.002), shape(BMO_SHAPE_PLANO, 0, 0.05, 0, 0.01), shape(BMO_SHAPE_CONVEX, 0, 0.052, 0, 0.01),
                group(BMO_SHAPE_UNION, 3, 2, 0.051), shape(BMO_SHAPE_BOX, 0, 0.1, 0, 0.005)};
    D.children = {0, 1, 2, 5, 4};
    D.objects = {object(BMO_OBJ_REFRACTIVE, 3, -1, -1, 0), object(BMO_OBJ_REFRACTIVE, 6, -1, -1, 0), object(BMO_OBJ_SPOTDETECTOR, 7, -1, -1, -1, -1, 0)};
    return D;
}
Desc asphere_scene() {
    Desc D;
    D.shapes = {group(BMO_SHAPE_ASPH_CONVEX, 0, 3, 0.0)};
    D.coefs = {1e-3, -2e-5, 3e-7};
    D.objects = {object(BMO_OBJ_REFRACTIVE, 0, -1, -1, 0)};
    return D;
}

// Latitude/longitude sphere of radius r around c: 2 * lon * (bands - 1) faces, 9 doubles each; `jitter` moves the vertices (seeded).
// `rot`: a row-major rotation applied about c.
std::vector<double> sphere_mesh(int bands, int lon, double r, const double c[3], double jitter, const double* rot = nullptr) {
    Rng rng{0x9E3779B97F4A7C15ull};
    std::vector<d3> ring((size_t)(bands + 1) * lon);
    for (int i = 0; i <= bands; ++i)
        for (int j = 0; j < lon; ++j) {
            const double th = 3.141592653589793 * i / bands, ph = 6.283185307179586 * j / lon;
            const double rr = r * (1.0 + jitter * (rng() - 0.5));
            d3 p{rr * jl::sin(th) * jl::cos(ph), rr * jl::cos(th), rr * jl::sin(th) * jl::sin(ph)};
            if (i == 0 || i == bands) p = d3{0, i == 0 ? r : -r, 0};  // the poles: one vertex each
            if (rot) p = d3{rot[0] * p.x + rot[1] * p.y + rot[2] * p.z, rot[3] * p.x + rot[4] * p.y + rot[5] * p.z, rot[6] * p.x + rot[7] * p.y + rot[8] * p.z};
            ring[(size_t)i * lon + j] = d3{p.x + c[0], p.y + c[1], p.z + c[2]};
        }
    std::vector<double> tris;
    auto face = [&](const d3& a, const d3& b, const d3& d) {
        for (const d3* v : {&a, &b, &d}) tris.insert(tris.end(), {v->x, v->y, v->z});
    };
    for (int i = 0; i < bands; ++i)
        for (int j = 0; j < lon; ++j) {
            const d3 &a = ring[(size_t)i * lon + j], &b = ring[(size_t)i * lon + (j + 1) % lon];
            const d3 &e = ring[(size_t)(i + 1) * lon + j], &f = ring[(size_t)(i + 1) * lon + (j + 1) % lon];
            if (i > 0) face(a, f, b);
            if (i < bands - 1) face(a, e, f);
        }
    return tris;
}
// A mirror with the given triangles as its MESH shape 0.
Desc mesh_scene(std::vector<double> tris, int flags = 0) {
    Desc D;
    bmo_shape s = shape(BMO_SHAPE_MESH, 0, 0, 0, 0.02);
    s.tri_count = (int32_t)(tris.size() / 9);
    s.flags = flags;
    D.shapes = {s};
    D.tris = std::move(tris);
    D.objects = {object(BMO_OBJ_MIRROR, 0)};
    return D;
}

unsigned long long fnv1a(const std::vector<char>& b) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for (char c : b) h = (h ^ (unsigned char)c) * 0x100000001b3ull;
    return h;
}
SceneImage build(const char* name, Desc& D) {
    SceneImage img;
    std::string err;
    const int rc = build_scene_image(D.finish(), img, err);
    CHECK(rc == BMO_OK, "%s: %d %s", name, rc, err.c_str());
    CHECK(img.blob.size() == img.hdr.total && img.blob.size() % 16 == 0, "%s: blob of %zu bytes, header says %u", name, img.blob.size(), img.hdr.total);
    std::printf("blob %-28s %10zu bytes  fnv1a %016llx\n", name, img.blob.size(), fnv1a(img.blob));
    return img;
}
void refused(const char* what, Desc D, int code) {
    SceneImage img;
    std::string err;
    const int rc = build_scene_image(D.finish(), img, err);
    CHECK(rc == code && err == what, "wanted %d \"%s\", got %d \"%s\"", code, what, rc, err.c_str());
}

// ---- BVH against brute force: (t, face) of 2 000 seeded rays on shape 0 of the scene viewed at `blob`; the two must agree bit for bit
struct Nearest {
    std::vector<double> t;
    std::vector<int32_t> fid;
    int hits = 0;
};
Nearest bvh_against_brute_force(const char* name, const char* blob, const BlobHeader& hdr, bool want_bvh) {
    const SceneView S = view_of(blob, &hdr);
    const bmo_shape& sh = S.shapes[0];
    CHECK(sh.kind == BMO_SHAPE_MESH && ((sh.flags & BMO_SHAPE_FLAG_BVH) != 0) == want_bvh, "%s: flags %d", name, sh.flags);
    Rng rng{0x243F6A8885A308D3ull};
    Nearest out;
    for (int i = 0; i < 2000; ++i) {
        const double* f = S.tris + 9 * (size_t)(sh.tri_begin + (int)(rng() * sh.tri_count));
        const d3 on_face{(f[0] + f[3] + f[6]) / 3, (f[1] + f[4] + f[7]) / 3, (f[2] + f[5] + f[8]) / 3};
        d3 pos{rng.in(-0.05, 0.05), rng.in(-0.05, 0.05), rng.in(-0.05, 0.05)}, dir{rng.in(-1, 1), rng.in(-1, 1), rng.in(-1, 1)};
        if (i % 4 == 1) pos = on_face;                                   // starts on a face
        if (i % 4 == 2) dir = sub3(on_face, pos);                         // aimed at a face
        if (i % 8 == 3) pos = d3{5 + pos.x, pos.y, pos.z}, dir.x = 1.0;  // far outside, flying away: misses the bounding sphere
        int32_t f0 = -1, f1 = -1;
        const double t0 = mesh_nearest(S, sh.tri_begin, sh.tri_count, pos, dir, f0);
        const double t1 = want_bvh ? mesh_nearest_bvh(S, sh.child_begin, sh.tri_begin, sh.tri_count, pos, dir, kinf(), f1) : t0;
        if (!want_bvh) f1 = f0;
        CHECK(std::memcmp(&t0, &t1, 8) == 0 && f0 == f1, "%s ray %d: brute force (%.17g, %d), BVH (%.17g, %d)", name, i, t0, f0, t1, f1);
        if (i % 8 == 3) CHECK(f0 < 0, "%s ray %d was to miss", name, i);
        out.t.push_back(t0), out.fid.push_back(f0), out.hits += f0 >= 0;
    }
    CHECK(out.hits > 400 && out.hits < 1900, "%s: %d of 2000 rays hit", name, out.hits);
    return out;
}

void check_valid_scenes() {
    Desc L = two_lens_scene();
    const SceneImage lens = build("two lenses", L);
    const SceneView S = view_of(lens.blob.data(), &lens.hdr);
    CHECK((S.shapes[3].flags & BMO_SHAPE_FLAG_CONSECUTIVE) && S.shapes[3].tri_begin == 0, "consecutive union: flags %d", S.shapes[3].flags);
    CHECK(!(S.shapes[6].flags & BMO_SHAPE_FLAG_CONSECUTIVE), "union of shapes 5, 4: flags %d", S.shapes[6].flags);
    CHECK(S.n_cands == 3 && S.children[3] == 5 && S.n_table[1] == 1.5 && !lens.hdr.has_bvh() && !lens.hdr.has_splitter, "two lenses: tables");
    CHECK(lens.bound[3] > 0.05 && lens.bound[3] < 0.2, "two lenses: bounding sphere of radius %g", lens.bound[3]);
    Desc A = asphere_scene();
    const SceneImage asph = build("asphere", A);
    const SceneView SA = view_of(asph.blob.data(), &asph.hdr);
    CHECK(asph.hdr.has_asphere == 1 && SA.coefs[0] == 1e-3 && SA.coefs[2] == 3e-7, "asphere: coefficients");
    const double c[3] = {0, 0, 0};
    Desc M64 = mesh_scene(sphere_mesh(5, 8, 0.02, c, 0.0));
    CHECK(M64.tris.size() == 64 * 9, "%zu faces", M64.tris.size() / 9);
    const SceneImage m64 = build("sphere mesh, 64 faces", M64);
    CHECK(m64.bvh[0].n_nodes > 0 && m64.hdr.has_bvh() == 1, "64 faces: %d BVH nodes", m64.bvh[0].n_nodes);
    bvh_against_brute_force("64 faces", m64.blob.data(), m64.hdr, true);
    std::vector<double> t63 = sphere_mesh(5, 8, 0.02, c, 0.0);
    t63.resize(63 * 9);
    Desc M63 = mesh_scene(t63);
    const SceneImage m63 = build("sphere mesh, 63 faces", M63);
    CHECK(m63.bvh[0].n_nodes == 0 && m63.hdr.has_bvh() == 0, "63 faces: %d BVH nodes", m63.bvh[0].n_nodes);
    bvh_against_brute_force("63 faces", m63.blob.data(), m63.hdr, false);
    Desc MN = mesh_scene(sphere_mesh(12, 16, 0.02, c, 0.2), BMO_SHAPE_FLAG_NO_BVH);
    const SceneImage mn = build("sphere mesh, NO_BVH", MN);
    CHECK(mn.bvh[0].n_nodes == 0 && mn.hdr.has_bvh() == 0, "NO_BVH: %d BVH nodes", mn.bvh[0].n_nodes);
    bvh_against_brute_force("NO_BVH", mn.blob.data(), mn.hdr, false);
    Desc MB = mesh_scene(sphere_mesh(12, 16, 0.02, c, 0.2), BMO_SHAPE_FLAG_BVH);  // (the output flag on input: ignored)
    const SceneImage mb = build("sphere mesh, 352 faces", MB);
    CHECK(mb.bvh[0].n_nodes > 40 && mb.bvh[0].depth <= BMO_BVH_MAX_DEPTH && mb.bvh[0].max_leaf <= BVH_MAX_LEAF, "352 faces: %d nodes", mb.bvh[0].n_nodes);
    bvh_against_brute_force("352 faces", mb.blob.data(), mb.hdr, true);
}

void check_refusals() {
    auto lens = [](std::function<void(Desc&)> f) {
        Desc D = two_lens_scene();
        f(D);
        return D;
    };
    auto desc = [&](std::function<void(bmo_scene_desc&)> f) { return lens([&](Desc& D) { D.tweak = f; }); };
    refused("abi version mismatch", desc([](bmo_scene_desc& d) { d.abi_version += 1; }), BMO_ERR_INVALID);
    refused("bad counts", desc([](bmo_scene_desc& d) { d.n_lambda = 0; }), BMO_ERR_INVALID);
    refused("bad counts", desc([](bmo_scene_desc& d) { d.n_objects = -1; }), BMO_ERR_INVALID);
    refused("unknown shape kind", lens([](Desc& D) { D.shapes[1].kind = BMO_SHAPE_KIND_COUNT; }), BMO_ERR_UNSUPPORTED);
    refused("child range out of bounds", lens([](Desc& D) { D.shapes[6].child_count = 3; }), BMO_ERR_INVALID);
    refused("child range out of bounds", lens([](Desc& D) { D.shapes[3].child_begin = -1; }), BMO_ERR_INVALID);
    refused("meniscus needs 3 children", lens([](Desc& D) { D.shapes[6].kind = BMO_SHAPE_MENISCUS; }), BMO_ERR_INVALID);
    refused("child id out of bounds", lens([](Desc& D) { D.children[4] = 8; }), BMO_ERR_INVALID);
    refused("nested union / mesh child", lens([](Desc& D) { D.children[3] = 3; }), BMO_ERR_INVALID);
    refused("nested meniscus", lens([](Desc& D) { D.shapes[3].kind = D.shapes[5].kind = BMO_SHAPE_MENISCUS, D.shapes[5].child_count = 3, D.children[0] = 5; }),
            BMO_ERR_INVALID);
    Desc A = asphere_scene();
    A.shapes[0].child_count = 4;
    refused("aspheric coefficient range out of bounds", std::move(A), BMO_ERR_INVALID);
    const double c[3] = {0, 0, 0};
    Desc M = mesh_scene(sphere_mesh(5, 8, 0.02, c, 0.0));
    M.shapes[0].tri_count += 1;
    refused("triangle range out of bounds", std::move(M), BMO_ERR_INVALID);
    Desc G = mesh_scene(sphere_mesh(5, 8, 0.02, c, 0.0));  // 60 M triangles stated, none there: refused before any triangle is read
    G.tweak = [](bmo_scene_desc& d) { d.n_tris = 60000000, d.tris = nullptr; };
    refused("scene blob larger than 4 GiB (32-bit table offsets): fewer triangles or smaller tables", std::move(G), BMO_ERR_INVALID);
    refused("unknown object kind", lens([](Desc& D) { D.objects[0].kind = BMO_OBJ_KIND_COUNT; }), BMO_ERR_UNSUPPORTED);
    refused("object shape id out of bounds", lens([](Desc& D) { D.objects[1].shape[0] = 8; }), BMO_ERR_INVALID);
    refused("medium id out of bounds", lens([](Desc& D) { D.objects[1].medium[1] = 1; }), BMO_ERR_INVALID);
    refused("refractive object without medium", lens([](Desc& D) { D.objects[0].medium[0] = -1; }), BMO_ERR_INVALID);
    refused("missing second medium", lens([](Desc& D) { D.objects[0].kind = BMO_OBJ_DOUBLET, D.objects[0].shape[1] = 6; }), BMO_ERR_INVALID);
    refused("detector slot out of bounds", lens([](Desc& D) { D.objects[2].detector = 1; }), BMO_ERR_INVALID);
}

void check_bvh_corner_cases() {
    std::vector<double> same;  // 100 faces around the origin whose boxes all have the origin as their centre: no SAH split, object medians
    for (int k = 0; k < 100; ++k) {
        const double s = 0.01 + 1e-4 * k;
        same.insert(same.end(), {-s, -s, -s, s, -s, s, 0.25 * s, s, -0.5 * s});
    }
    Desc C = mesh_scene(same);
    const SceneImage one = build("faces of one centre", C);
    CHECK(one.bvh[0].n_nodes > 0 && one.bvh[0].max_leaf <= BVH_MAX_LEAF, "one centre: %d nodes, leaves of %d", one.bvh[0].n_nodes, one.bvh[0].max_leaf);
    bvh_against_brute_force("one centre", one.blob.data(), one.hdr, true);
    const double c[3] = {0, 0, 0};
    std::vector<double> bad = sphere_mesh(12, 16, 0.02, c, 0.2);
    bad[9 * 200 + 4] = std::nan("");
    std::vector<BvhNode> nodes;
    std::vector<int32_t> faces;
    BvhStats st;
    CHECK(bvh_build(bad.data(), (int)(bad.size() / 9), 1e-9, nodes, faces, st) == -1 && nodes.empty() && faces.empty(), "a non-finite vertex: no BVH");
    Desc N = mesh_scene(bad);
    const SceneImage nan = build("mesh with a NaN vertex", N);
    CHECK(nan.bvh[0].n_nodes == 0 && nan.hdr.has_bvh() == 0, "NaN vertex: %d BVH nodes", nan.bvh[0].n_nodes);
    CHECK(!(view_of(nan.blob.data(), &nan.hdr).shapes[0].flags & BMO_SHAPE_FLAG_BVH), "NaN vertex: the mesh stays brute force");
    for (double keps : {0.0, -1e-9}) {
        Desc K = mesh_scene(sphere_mesh(12, 16, 0.02, c, 0.2));
        K.mt_keps = keps;
        const SceneImage k = build(keps == 0.0 ? "mt_keps = 0" : "mt_keps < 0", K);
        CHECK(k.bvh[0].n_nodes == 0 && k.hdr.has_bvh() == 0 && !(view_of(k.blob.data(), &k.hdr).shapes[0].flags & BMO_SHAPE_FLAG_BVH), "mt_keps = %g: no BVH", keps);
    }
}

void check_sweep_merge() {
    // exact rotations (Pythagorean triples: no libm in them) of a jittered sphere that sits off the origin
    const double rots[3][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0.6, -0.8, 0, 0.8, 0.6, 0, 0, 0, 1}, {1, 0, 0, 0, 5.0 / 13, -12.0 / 13, 0, 12.0 / 13, 5.0 / 13}};
    const double c[3] = {0.004, -0.003, 0.002};
    Desc D[3];
    std::vector<bmo_scene_desc> descs;
    std::vector<Nearest> own;
    std::vector<int> n_nodes;
    for (int q = 0; q < 3; ++q) {
        D[q] = mesh_scene(sphere_mesh(12, 16, 0.02, c, 0.6, rots[q]));
        const SceneImage one = build(q == 0 ? "sweep configuration 0" : (q == 1 ? "sweep configuration 1" : "sweep configuration 2"), D[q]);
        own.push_back(bvh_against_brute_force("sweep configuration", one.blob.data(), one.hdr, true));
        n_nodes.push_back(one.bvh[0].n_nodes);
        descs.push_back(D[q].d);
    }
    std::printf("sweep: BVH nodes %d, %d, %d\n", n_nodes[0], n_nodes[1], n_nodes[2]);
    CHECK(n_nodes[0] != n_nodes[1] && n_nodes[1] != n_nodes[2] && n_nodes[0] != n_nodes[2], "the rotations were to give node tables of different sizes");
    const auto e_descs = exact(descs);
    SceneImage all;
    std::string err;
    const int rc = merge_sweep_images(e_descs.get(), 3, all, err);
    CHECK(rc == BMO_OK, "merge: %d %s", rc, err.c_str());
    CHECK(all.n_configs == 3 && all.stride % 256 == 0 && all.stride >= all.hdr.total && all.blob.size() == 3 * all.stride, "merge: stride %llu", (unsigned long long)all.stride);
    std::printf("blob %-28s %10zu bytes  fnv1a %016llx\n", "sweep of 3", all.blob.size(), fnv1a(all.blob));
    for (int q = 0; q < 3; ++q) {
        const char* slice = all.blob.data() + all.stride * (uint64_t)q;
        CHECK(std::memcmp(slice, &all.hdr, sizeof all.hdr) == 0, "configuration %d: its slice starts with the common header", q);
        const Nearest got = bvh_against_brute_force("sweep slice", slice, all.hdr, true);
        CHECK(got.t.size() == own[(size_t)q].t.size() && std::memcmp(got.t.data(), own[(size_t)q].t.data(), 8 * got.t.size()) == 0 && got.fid == own[(size_t)q].fid,
              "configuration %d: the slice gives other hits than the configuration built alone", q);
    }
    D[2].shapes[0].tri_count -= 1;  // a change of topology
    descs[2] = *D[2].finish();
    const auto e_changed = exact(descs);
    SceneImage none;
    CHECK(merge_sweep_images(e_changed.get(), 3, none, err) == BMO_ERR_INVALID && err.find("configuration 2 differs from configuration 0 in shapes[0].tri_count") != std::string::npos,
          "topology change: %s", err.c_str());
}

}  // namespace

int main() {
    check_valid_scenes();
    check_refusals();
    check_bvh_corner_cases();
    check_sweep_merge();
    std::printf("scene_check ok\n");
    return 0;
}
