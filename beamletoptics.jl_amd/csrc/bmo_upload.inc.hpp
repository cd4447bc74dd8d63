// bmo_upload.inc.hpp — a ray batch on its way to the device (included by bmo_engine.hip inside its anonymous namespace, behind the
// handle structs; shares its pools and error helpers).  batch_upload at the end is the driver, behind bmo_batch_upload and
// bmo_trace_sweep; everything above it is one phase, with the kernels it launches:
//   root_key_kernel, root_chord_kernel, root_order_key_kernel, root_ring_jump_kernel, bin_planes_kernel
//   check_batch, copy_batch               the batch's shape, its planes and wavelength indices on the device
//   RootKeys, sort_roots, bin_planes      the permutation of the roots by their keys, the planes in that order
//   root_order_wanted                     the order asked for (Switches::root_order)
//   order_by_chords, order_by_masks       the two kinds of keys (and auto's test of the bundle's own order)

// Coherence key of a root ray: the set of candidates (first 64 of the candidate table) whose bounding sphere the ray's line meets —
// what the mask pre-pass of trace_all computes for the first bounce.  Rays with equal keys walk the same slots, so putting them next
// to each other makes waves whose lanes agree on the shape they march (bmo_lane.hpp "scalar scene access": one waterfall pass).
__global__ void root_key_kernel(const char* __restrict__ blob, BlobHeader hdr, const double* __restrict__ planes, int64_t n, unsigned long long* __restrict__ keys,
                                int32_t* __restrict__ ids) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const SceneView S = view_of(blob, &hdr);
    const d3 pos{planes[0 * n + j], planes[1 * n + j], planes[2 * n + j]}, dir{planes[3 * n + j], planes[4 * n + j], planes[5 * n + j]};
    unsigned long long mask = 0;
    const int nc = S.n_cands < 64 ? S.n_cands : 64;
    for (int i = 0; i < nc; ++i) {
        const BMO_KONST Cand& cd = S.cands[i];
        mask |= (unsigned long long)!cull_miss(cd.cx, cd.cy, cd.cz, cd.R, pos, dir) << i;
    }
    keys[j] = mask;
    ids[j] = (int32_t)j;
}

// Coherence order of the root rays (round 4).  A wave works on one shape at a time and a level of a wave lasts as long as its slowest
// lane, so the 64 rays of a wave should be NEIGHBOURS IN RAY SPACE — same elements, similar marches, ending together.  Bundle order does not
// give that: a disc source numbers its rays along a spiral (BeamGroups.jl:232-243: equal radius, every azimuth) and draws directions at random.
// A ray's line is described by the two points where it enters and leaves the scene's bounding sphere (the two-sphere parametrisation of a
// light field: position and direction weigh in with the leverage they have over the scene, no scale to choose); the rays are sorted by a
// Morton code over those six coordinates, scaled to the bundle's own extent.  In front of the code sits the ray's distance from the bundle's
// middle in that space, farthest first: the marginal rays are the ones that graze barrels and rims — marches of 500 - 1 000 evaluations,
// one dependent chain of ~1 ms each — and a launch ends when its slowest wave does, so they have to START first (the hardware hands out
// workgroups in index order).  Beam nodes keep the bundle's numbering: result order, detector order and retrace do not see any of this.
__global__ void root_chord_kernel(const double* __restrict__ planes, int64_t n, double cx, double cy, double cz, double R, double* __restrict__ chord) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double px = planes[0 * n + j], py = planes[1 * n + j], pz = planes[2 * n + j], dx = planes[3 * n + j], dy = planes[4 * n + j], dz = planes[5 * n + j];
    const double ox = cx - px, oy = cy - py, oz = cz - pz;
    const double dd = dx * dx + dy * dy + dz * dz, b = ox * dx + oy * dy + oz * dz, cc = ox * ox + oy * oy + oz * oz - R * R;
    const double disc = b * b - dd * cc;
    double e[6] = {cx, cy, cz, cx, cy, cz};  // (a line that misses the sphere meets nothing: it sorts to the middle, where it disturbs nobody)
    if (dd > 0.0 && disc >= 0.0) {
        const double sq = sqrt(disc), t0 = (b - sq) / dd, t1 = (b + sq) / dd;
        e[0] = px + t0 * dx, e[1] = py + t0 * dy, e[2] = pz + t0 * dz;
        e[3] = px + t1 * dx, e[4] = py + t1 * dy, e[5] = pz + t1 * dz;
    }
    for (int q = 0; q < 6; ++q) chord[q * n + j] = (e[q] == e[q]) ? e[q] : (q % 3 == 0 ? cx : (q % 3 == 1 ? cy : cz));
}
// lim[0..5] minima, lim[6..11] maxima of the six chord coordinates over the bundle
__global__ void root_order_key_kernel(const double* __restrict__ chord, int64_t n, const double* __restrict__ lim, unsigned long long* __restrict__ keys, int32_t* __restrict__ ids) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    unsigned long long key = 0;
    double far2 = 0.0;
    for (int g = 0; g < 2; ++g) {  // entry points, exit points: one scale per point set (isotropic)
        double hw = 0.0, mid[3];
        for (int a = 0; a < 3; ++a) {
            const double lo = lim[3 * g + a], hi = lim[6 + 3 * g + a];
            mid[a] = 0.5 * (lo + hi);
            hw = fmax(hw, 0.5 * (hi - lo));
        }
        double r2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double u = hw > 0.0 ? (chord[(3 * g + a) * n + j] - mid[a]) / hw : 0.0;  // [-1, 1]
            r2 += u * u;
            int q = (int)floor(u * 512.0 + 512.0);
            q = q < 0 ? 0 : (q > 1023 ? 1023 : q);
            unsigned long long v = (unsigned long long)q, sp = 0;
            for (int bit = 0; bit < 10; ++bit) sp |= ((v >> bit) & 1ull) << (6 * bit);
            key |= sp << (3 * g + a);
        }
        far2 = fmax(far2, r2);
    }
    // 16 coarse rings around the middle of the bundle in front of the code, outermost first (measured: the ragged config-2 bundle 9.0 ms
    // with them, 9.7 ms without; finer rings cost the multi-train scene 10 %): marginal rays — the ones that graze barrels — sit together
    // and start first when no feedback orders the tiles yet
    int ring = (int)(sqrt(far2) * 12.0);
    ring = ring > 15 ? 15 : ring;
    keys[j] = ((unsigned long long)(15 - ring) << 60) | key;
    ids[j] = (int32_t)j;
}
// Is the bundle's OWN numbering coherent already?  A disc source numbers its rays along a spiral (BeamGroups.jl:232-243): neighbours in the
// bundle sit at the same distance from the bundle's axis at every azimuth, and in a system that is close to rotationally symmetric about
// that axis such rays share their path exactly — 64 of them make a better wave than any patch of the Morton code (1/30 of the bundle wide in
// radius): SURVEY 8(d)'s collimated disc runs 40 % slower in Morton order.  Measure: the mean jump, from one ray to the next in bundle order,
// of the entry point's distance from the middle of the bundle's entry points (in units of the bundle's half width).  sum[0] += the jumps.
__global__ void root_ring_jump_kernel(const double* __restrict__ chord, int64_t n, const double* __restrict__ lim, double* __restrict__ sum) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double hw = 0.0, mid[3];
    for (int a = 0; a < 3; ++a) {
        mid[a] = 0.5 * (lim[a] + lim[6 + a]);
        hw = fmax(hw, 0.5 * (lim[6 + a] - lim[a]));
    }
    double jump = 0.0;
    if (j + 1 < n && hw > 0.0) {
        double r[2];
        for (int q = 0; q < 2; ++q) {
            double r2 = 0.0;
            for (int a = 0; a < 3; ++a) {
                const double u = (chord[a * n + j + q] - mid[a]) / hw;
                r2 += u * u;
            }
            r[q] = sqrt(r2);
        }
        jump = fabs(r[1] - r[0]);
    }
    for (int off = 32; off > 0; off >>= 1) jump += __shfl_down(jump, off);
    if ((threadIdx.x & 63) == 0 && jump != 0.0) atomicAdd(sum, jump);
}
// the batch's planes in slot order: out[p][s] = in[p][perm[s]]
__global__ void bin_planes_kernel(const double* __restrict__ in, const int32_t* __restrict__ perm, int64_t n, int n_planes, double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t j = perm[s];
    for (int p = 0; p < n_planes; ++p) out[(int64_t)p * n + s] = in[(int64_t)p * n + j];
}

// ---- check the batch
int check_batch(const bmo_scene* scene, const bmo_ray_batch* in, int32_t device) {
    if (in->kind != BMO_BEAM_RAY && in->kind != BMO_BEAM_POLARIZED && in->kind != BMO_BEAM_GAUSSIAN) return fail(BMO_ERR_INVALID, "bad beam kind");
    const int want = in->kind == BMO_BEAM_RAY ? BMO_PLANES_RAY : (in->kind == BMO_BEAM_POLARIZED ? BMO_PLANES_POLARIZED : BMO_PLANES_GAUSSIAN);
    const bool continued = in->kind == BMO_BEAM_GAUSSIAN && in->n_planes == BMO_PLANES_GAUSSIAN_CONTINUED;
    if ((in->n_planes != want && !continued) || in->n < 0) return fail(BMO_ERR_INVALID, "bad plane count");
    if (in->n > 0x7fffffff / 4) return fail(BMO_ERR_INVALID, "batch too large for one device (shard it)");
    for (int64_t i = 0; i < in->n; ++i)
        if (in->lambda_idx[i] < 0 || in->lambda_idx[i] >= scene->hdr.n_lambda) return fail(BMO_ERR_INVALID, "lambda_idx out of range");
    int ndev = bmo_device_count();
    if (ndev <= 0) return fail(BMO_ERR_NO_DEVICE, "no HIP device: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(BMO_ERR_INVALID, "bad device ordinal");
    return BMO_OK;
}

// ---- copy planes and wavelength indices
int copy_batch(const bmo_ray_batch* in, int32_t device, bmo_device_batch* b) {
    b->device = device;
    b->kind = in->kind;
    b->n = in->n;
    b->n_planes = in->n_planes;
    int rc;
    if ((rc = b->planes.alloc((size_t)in->n * in->n_planes * 8)) || (rc = b->li.alloc((size_t)in->n * 4))) return rc;
    if (in->n) {
        HIP_TRY(hipMemcpy(b->planes.p, in->planes, (size_t)in->n * in->n_planes * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->li.p, in->lambda_idx, (size_t)in->n * 4, hipMemcpyHostToDevice));
    }
    return BMO_OK;
}

// ---- sort the permutation and bin the planes: what both orders do with their keys.  The number of key bits, what happens between the
// two steps and the synchronisation behind them (the temporaries go back to the pool) stay with the caller.
struct RootKeys {
    DevBuf keys, keys_out, ids;
    int alloc(bmo_device_batch* b) {
        const size_t n = (size_t)b->n;
        int rc;
        if ((rc = keys.alloc(n * 8)) || (rc = keys_out.alloc(n * 8)) || (rc = ids.alloc(n * 4)) || (rc = b->perm.alloc(n * 4))) return rc;
        return BMO_OK;
    }
};
// b->perm = the root ids in the order of the low `bits` bits of their keys (a stable sort: bundle order within a key)
int sort_roots(RootKeys& k, bmo_device_batch* b, int bits, Temps& tmp) {
    CUB_TRY(tmp, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const unsigned long long*)k.keys.p, (unsigned long long*)k.keys_out.p, (const int32_t*)k.ids.p,
                                                    (int32_t*)b->perm.p, (int)b->n, 0, bits, nullptr));
    return BMO_OK;
}
int bin_planes(bmo_device_batch* b) {
    if (int rc = b->binned.alloc((size_t)b->n * b->n_planes * 8)) return rc;
    hipLaunchKernelGGL(bin_planes_kernel, dim3((unsigned)((b->n + 255) / 256)), dim3(256), 0, nullptr, (const double*)b->planes.p, (const int32_t*)b->perm.p, b->n,
                       b->n_planes, (double*)b->binned.p);
    return BMO_OK;
}

// ---- choose the order.  BMO_ROOT_ORDER = chord (root_order_key_kernel) | mask (round 3's candidate-set keys) | none; unset: auto, which is
// chord unless the bundle's own numbering turns out coherent (order_by_chords), and mask where the scene has no bound to take chords through.
std::string root_order_wanted(bool order_roots, const char* order_env) {
    return !order_roots ? "none" : (order_env ? order_env : "auto");
}

// ---- make the keys: chords.  `root_order` is "chord" or "auto" and says on return what was done: "chord", or "mask" when auto found the
// bundle's own numbering coherent (it is kept, + the candidate-set bins of order_by_masks).
int order_by_chords(const bmo_scene* scene, bmo_device_batch* b, std::string& root_order) {
    const int64_t n = b->n;
    DevBuf chord, lim;
    RootKeys k;
    Temps tmp;  // (the reductions and the sort share its scratch block)
    int rc;
    if ((rc = chord.alloc((size_t)n * 6 * 8)) || (rc = lim.alloc(13 * 8)) || (rc = k.alloc(b))) return rc;
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(root_chord_kernel, dim3(nb), dim3(256), 0, nullptr, (const double*)b->planes.p, n, scene->bound[0], scene->bound[1], scene->bound[2],
                       scene->bound[3], (double*)chord.p);
    for (int q = 0; q < 6; ++q) {
        CUB_TRY(tmp, hipcub::DeviceReduce::Min(cub_tmp, cub_bytes, (const double*)chord.p + (size_t)q * n, (double*)lim.p + q, (int)n, nullptr));
        CUB_TRY(tmp, hipcub::DeviceReduce::Max(cub_tmp, cub_bytes, (const double*)chord.p + (size_t)q * n, (double*)lim.p + 6 + q, (int)n, nullptr));
    }
    if (root_order == "auto") {
        double jump = 0.0;
        HIP_TRY(hipMemsetAsync((double*)lim.p + 12, 0, 8, nullptr));
        hipLaunchKernelGGL(root_ring_jump_kernel, dim3(nb), dim3(256), 0, nullptr, (const double*)chord.p, n, (const double*)lim.p, (double*)lim.p + 12);
        HIP_TRY(hipMemcpy(&jump, (const double*)lim.p + 12, 8, hipMemcpyDeviceToHost));
        const bool own_order = jump / (double)n < 0.01;  // (a spiral: ~1e-6; positions or directions drawn at random: ~0.3)
        DBG("root order: mean ring jump %.3g -> %s", jump / (double)n, own_order ? "the bundle's own order" : "Morton order of the chords");
        if (own_order) {
            b->perm.release();
            root_order = "mask";
            return BMO_OK;
        }
    }
    root_order = "chord";
    hipLaunchKernelGGL(root_order_key_kernel, dim3(nb), dim3(256), 0, nullptr, (const double*)chord.p, n, (const double*)lim.p, (unsigned long long*)k.keys.p,
                       (int32_t*)k.ids.p);
    if ((rc = sort_roots(k, b, 64, tmp)) || (rc = bin_planes(b))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // the temporaries go back to the pool
    HIP_TRY(hipGetLastError());
    return BMO_OK;
}

// ---- make the keys: candidate-set masks.  A bundle whose rays all have one key — a single disc source aimed at one train — keeps its
// order and costs nothing later.
int order_by_masks(bmo_scene* scene, bmo_device_batch* b) {
    int rc = BMO_OK;
    const char* dblob = scene->device_blob(b->device, rc);
    if (rc) return rc;
    const int64_t n = b->n;
    RootKeys k;
    Temps tmp;
    if ((rc = k.alloc(b))) return rc;
    hipLaunchKernelGGL(root_key_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, dblob, scene->hdr, (const double*)b->planes.p, n,
                       (unsigned long long*)k.keys.p, (int32_t*)k.ids.p);
    if ((rc = sort_roots(k, b, std::min(64, std::max(1, scene->hdr.n_cands)), tmp))) return rc;
    unsigned long long k0 = 0, k1 = 0;
    HIP_TRY(hipMemcpy(&k0, k.keys_out.p, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&k1, (const char*)k.keys_out.p + (size_t)(n - 1) * 8, 8, hipMemcpyDeviceToHost));
    if (k0 == k1) {
        b->perm.release();  // one key: nothing to bin
        return BMO_OK;
    }
    if ((rc = bin_planes(b))) return rc;
    HIP_TRY(hipDeviceSynchronize());  // the sort's temporaries go back to the pool
    return BMO_OK;
}

// Roots are binned by coherence key once, here.  Ordering only engages from 4 096 rays and in a scene that has candidates.
// order_roots: off for sweeps (the scene bound and the candidate masks are per configuration).
int batch_upload(bmo_scene* scene, const bmo_ray_batch* in, int32_t device, bmo_device_batch** out, bool order_roots) {
    if (!scene || !in || !out) return fail(BMO_ERR_INVALID, "null argument");
    int rc;
    if ((rc = check_batch(scene, in, device))) return rc;
    HIP_TRY(hipSetDevice(device));
    auto b = std::make_unique<bmo_device_batch>();
    if ((rc = copy_batch(in, device, b.get()))) return rc;
    std::string root_order = root_order_wanted(order_roots, read_switches().root_order);  // (read at every upload, with the per-solve names: one reader, and an upload is no hot path)
    const bool large = in->n >= 4096 && scene->hdr.n_cands > 0;
    if (large && scene->bound[3] > 0.0 && (root_order == "chord" || root_order == "auto")) {
        if ((rc = order_by_chords(scene, b.get(), root_order))) return rc;  // (leaves "chord", or "mask": auto kept the bundle's own order)
    }
    if (root_order == "auto") root_order = "mask";  // (no bound to take chords through)
    if (large && root_order == "mask") {
        if ((rc = order_by_masks(scene, b.get()))) return rc;
    }
    *out = b.release();
    return BMO_OK;
}
