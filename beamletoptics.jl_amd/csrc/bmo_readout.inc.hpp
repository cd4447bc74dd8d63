// bmo_readout.inc.hpp — detector read-out kernels (included by bmo_engine.hip; shares its pool / error helpers).
//
// Every read-out is one split-and-reduce pipeline: a grid of points times the recorded rows of a detector slot, summed per configuration.
//   * The rows of configuration c are the consecutive range begin[c] .. begin[c] + count[c] - 1 of the slot (slot_ranges).  A single call is
//     the K = 1 case: one configuration that owns every row.
//   * SplitPlan cuts each range into splits (psf_splits / pd_splits: enough workgroups to fill the chip) and lists them as flat work items
//     {h0, h1, cfg}; a configuration without rows has none.  Consecutive configurations whose items fit the grid's y limit and 1 GiB of
//     partial sums form one launch.
//   * An accumulate kernel (psf_accumulate_list_kernel / pd_field_kernel) runs one workgroup per (256 grid points, work item) and writes the
//     item's partial sum to row `item - w0` of a [item][point] plane; reduce_splits_kernel sums each configuration's rows in split order
//     and finishes (PSF: abs2, and the field when asked; Photodetector: added to the caller's field).  The result is deterministic for given
//     (grid, counts); it re-associates the reference's sequential sum at split boundaries only.
//   * The plan, the poses and the axes go up in one copy (Packed); one pair of events times the launches (EventTimer).
//   * One exception: a PSF launch of one configuration runs psf_accumulate_kernel, the same sum with the split and the pose in the kernel
//     arguments instead of the lists (see there).
//
// PSF intensity (PSFDetector.jl:190-237): an n x n grid of sample points times H recorded hits, one cis() per pair.
//   * a workgroup owns 256 consecutive grid points (point index = i + n*j, i fastest like the reference's Matrix); the hits of its split
//     are staged through LDS in tiles of 256 x 9 doubles so every lane reads each hit from LDS (broadcast reads) instead of HBM;
//   * arithmetic follows the reference expression by expression (p = origin + x*e1 + z*e2; l = dot(p - hit, dir);
//     phase = k*(opl + l); acc += proj*cis(phase)), FP64, no contraction.
namespace {

constexpr int PSF_TILE = 256;

// origin + x * e1 + z * e2 (left to right): the point (x, z) of the detector plane
__device__ __forceinline__ d3 psf_point(const d3& origin, const d3& e1, const d3& e2, double x, double z) {
    return d3{(origin.x + x * e1.x) + z * e2.x, (origin.y + x * e1.y) + z * e2.y, (origin.z + x * e1.z) + z * e2.z};
}
// opl + l of row r seen from p, l = dot(p - hit, dir): the path whose k-fold is the phase of the row at p
__device__ __forceinline__ double psf_path(const d3& p, const double* r) {
    const double l = ((p.x - r[0]) * r[3] + (p.y - r[1]) * r[4]) + (p.z - r[2]) * r[5];
    return r[6] + l;
}
// rows base .. base + cnt - 1 staged into `tile` with coalesced loads; every lane of the workgroup calls it (it syncs)
__device__ __forceinline__ void psf_stage_rows(const double* __restrict__ hits, int64_t base, int cnt, double* tile) {
    __syncthreads();
    for (int q = threadIdx.x; q < cnt * 9; q += 256) tile[q] = hits[base * 9 + q];
    __syncthreads();
}

// The point-pt term of the workgroup's grid (psf_point of its axes) summed over hits h0 .. h1 - 1 in hit order.  Every lane of the
// workgroup calls it (it stages the hits through `tile` and syncs); a lane past the grid (`live` false) only helps to load.
__device__ __forceinline__ double2 psf_sum_range(const double* __restrict__ hits, int64_t h0, int64_t h1, const double* __restrict__ xs,
                                                 const double* __restrict__ zs, int32_t n, int64_t pt, bool live, const d3& origin, const d3& e1,
                                                 const d3& e2, double* tile) {
    d3 p{0, 0, 0};
    if (live) p = psf_point(origin, e1, e2, xs[(int)(pt % n)], zs[(int)(pt / n)]);
    double re = 0.0, im = 0.0;
    for (int64_t base = h0; base < h1; base += PSF_TILE) {
        const int cnt = (int)(h1 - base < PSF_TILE ? h1 - base : PSF_TILE);
        psf_stage_rows(hits, base, cnt, tile);
        if (live) {
            for (int h = 0; h < cnt; ++h) {
                const double* r = tile + 9 * h;
                const double phase = r[8] * psf_path(p, r);
                double s, c;
                sincos(phase, &s, &c);
                re += r[7] * c;
                im += r[7] * s;
            }
        }
    }
    return make_double2(re, im);
}

// One split of one configuration: rows h0 .. h1 - 1 of the slot.  Configuration c owns items first_work .. first_work + n_splits - 1.
struct SplitWork {
    int64_t h0, h1;
    int32_t cfg, pad;
};
struct SplitCfg {
    int64_t first_work;
    int32_t n_splits, pad;  // 0: no rows
};
struct PsfPose {
    d3 origin, e1, e2;
};

// A launch of one configuration, which every single call is: split blockIdx.y of its n_hits rows, the pose in the kernel arguments.  It does
// what the list kernel below does for such a launch; it stays because its code is the faster one where a call has few workgroups and waits
// on latency (the loop of 1 024-row calls of tools/psf_sweep_bench.py: 2.5 % less kernel time, profiles/readout_refactor_ab.txt).
__global__ __launch_bounds__(256) void psf_accumulate_kernel(const double* __restrict__ hits, int64_t n_hits, int64_t hits_per_split, const double* __restrict__ xs,
                                                             const double* __restrict__ zs, int32_t n, d3 origin, d3 e1, d3 e2, double2* __restrict__ partial) {
    __shared__ double tile[PSF_TILE * 9];
    const int64_t n_pts = (int64_t)n * n;
    const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = pt < n_pts;
    const int64_t h0 = (int64_t)blockIdx.y * hits_per_split;
    const int64_t h1 = h0 + hits_per_split < n_hits ? h0 + hits_per_split : n_hits;
    const double2 v = psf_sum_range(hits, h0, h1, xs, zs, n, pt, live, origin, e1, e2, tile);
    if (live) partial[(int64_t)blockIdx.y * n_pts + pt] = v;
}

// work item w0 + blockIdx.y, on its configuration's axes (xs, zs: [K][n]) and pose
__global__ __launch_bounds__(256) void psf_accumulate_list_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, int64_t w0,
                                                                  const PsfPose* __restrict__ pose, const double* __restrict__ xs,
                                                                  const double* __restrict__ zs, int32_t n, double2* __restrict__ partial) {
    __shared__ double tile[PSF_TILE * 9];
    const int64_t n_pts = (int64_t)n * n;
    const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = pt < n_pts;
    const SplitWork W = work[w0 + blockIdx.y];
    const PsfPose& C = pose[W.cfg];
    const double2 v = psf_sum_range(hits, W.h0, W.h1, xs + (int64_t)W.cfg * n, zs + (int64_t)W.cfg * n, n, pt, live, C.origin, C.e1, C.e2, tile);
    if (live) partial[(int64_t)blockIdx.y * n_pts + pt] = v;
}

// what becomes of the sum (re, im) of point i = c * n_pts + pt
struct PsfFinish {
    double* intensity;
    double2* field;  // nullptr: not asked for
    __device__ void operator()(int64_t i, double re, double im) const {
        intensity[i] = re * re + im * im;  // abs2
        if (field) field[i] = make_double2(re, im);
    }
};
struct PdFinish {
    double2* field;  // the caller's: added to
    __device__ void operator()(int64_t i, double re, double im) const {
        double2* f = field + i;
        *f = make_double2(f->x + re, f->y + im);
    }
};

// configuration c0 + blockIdx.y: its splits (partial rows first_work - w0 ...) summed in split order; none: the sum is +0
template <class Finish>
__global__ void reduce_splits_kernel(const SplitCfg* __restrict__ cfg, int32_t c0, int64_t w0, const double2* __restrict__ partial, int64_t n_pts, Finish finish) {
    const int64_t pt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pt >= n_pts) return;
    const int32_t c = c0 + (int32_t)blockIdx.y;
    const SplitCfg& C = cfg[c];
    double re = 0.0, im = 0.0;
    for (int s = 0; s < C.n_splits; ++s) {
        const double2 v = partial[(C.first_work - w0 + s) * n_pts + pt];
        re += v.x;
        im += v.y;
    }
    finish((int64_t)c * n_pts + pt, re, im);
}

// configuration of rows first_row + stride * h of the slot (det_node -> node -> root -> root_cfg)
__global__ void row_cfg_kernel(const int32_t* __restrict__ det_node, int64_t first_row, int64_t stride, int64_t n, const int32_t* __restrict__ order,
                               const int32_t* __restrict__ root, const int32_t* __restrict__ root_cfg, int32_t* __restrict__ out) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n) return;
    out[h] = root_cfg[root[order[det_node[first_row + stride * h]]]];
}

}  // namespace

// workgroup rows of the sum of n_hits hits on a grid of pt_blocks x 256 points: enough workgroups to fill 256 CUs several times over, but
// never splits shorter than one LDS tile
// (tests/readout_ref.py restates this function, pd_splits below and SplitPlan's launches, to assert which path a test shape takes;
// tests/test_readout_reference.py reads PSF_TILE and the two workgroup targets, 4096 and 2048, from this text: keep them in step)
static void psf_splits(int64_t n_hits, unsigned pt_blocks, int64_t& n_splits, int64_t& hits_per_split) {
    n_splits = (4096 + pt_blocks - 1) / pt_blocks;
    const int64_t max_splits = (n_hits + PSF_TILE - 1) / PSF_TILE;
    if (n_splits > max_splits) n_splits = max_splits;
    if (n_splits < 1) n_splits = 1;
    if (n_splits > 65535) n_splits = 65535;
    hits_per_split = (n_hits + n_splits - 1) / n_splits;
    hits_per_split = (hits_per_split + PSF_TILE - 1) / PSF_TILE * PSF_TILE;
    if (hits_per_split < PSF_TILE) hits_per_split = PSF_TILE;
    n_splits = n_hits > 0 ? (n_hits + hits_per_split - 1) / hits_per_split : 1;
}
// workgroup rows of the field sum of H beamlets on a grid of pt_blocks x 256 points: enough ranges to fill the chip when the grid is small
static void pd_splits(int64_t H, unsigned pt_blocks, int64_t& n_splits, int64_t& hits_per_split) {
    n_splits = (2048 + pt_blocks - 1) / pt_blocks;
    if (n_splits > H) n_splits = H;
    if (n_splits > 65535) n_splits = 65535;
    if (n_splits < 1) n_splits = 1;
    hits_per_split = (H + n_splits - 1) / n_splits;
    n_splits = (H + hits_per_split - 1) / hits_per_split;
}

// A pair of events around the launches of a read-out; destroyed on every path.
struct EventTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st = 0;
    int start(hipStream_t stream) {
        st = stream;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, st));
        return BMO_OK;
    }
    // waits for everything queued so far; ms: nullptr if not asked for
    int stop(double* ms) {
        HIP_TRY(hipEventRecord(e1, st));
        HIP_TRY(hipEventSynchronize(e1));
        HIP_TRY(hipGetLastError());
        float f = 0;
        HIP_TRY(hipEventElapsedTime(&f, e0, e1));
        if (ms) *ms = f;
        return BMO_OK;
    }
    ~EventTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    EventTimer() = default;
    EventTimer(const EventTimer&) = delete;
    EventTimer& operator=(const EventTimer&) = delete;
};

// Small host arrays that go to the device in one buffer and one copy (a single call pays one upload for its plan, pose and axes).
struct Packed {
    std::vector<char> host;
    DevBuf dev;
    template <class T>
    size_t add(const T* v, size_t count) {  // its offset, for at()
        const size_t off = host.size(), bytes = count * sizeof(T);
        host.resize(off + (bytes + 7) / 8 * 8);
        if (bytes) memcpy(host.data() + off, v, bytes);
        return off;
    }
    template <class T>
    size_t add(const std::vector<T>& v) { return add(v.data(), v.size()); }
    int upload(hipStream_t st) {
        if (int rc = dev.alloc(host.size())) return rc;
        if (!host.empty()) HIP_TRY(hipMemcpyAsync(dev.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
        return BMO_OK;
    }
    template <class T>
    const T* at(size_t off) const { return (const T*)((const char*)dev.p + off); }
};

// rows begin[c] .. begin[c] + count[c] - 1 (units of `stride` rows, relative to the slot's first) belong to configuration c
struct Ranges {
    std::vector<int64_t> begin, count;
};
// The ranges of the H units of slot `detector`.  per_config: the result is a sweep's and each unit goes to its root's configuration (units
// of one configuration are consecutive: rows are in root order, roots in configuration order); otherwise one configuration owns them all.
static int slot_ranges(bmo_trace_result* res, int32_t detector, int64_t stride, int64_t H, int32_t K, bool per_config, const char* refusal, hipStream_t st, Ranges& R) {
    R.begin.assign((size_t)K, 0);
    R.count.assign((size_t)K, 0);
    if (!per_config) {
        R.count[0] = H;
        return BMO_OK;
    }
    DevBuf row_cfg;
    if (int rc = row_cfg.alloc((size_t)H * 4)) return rc;
    hipLaunchKernelGGL(row_cfg_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, st, (const int32_t*)res->det_node.p, res->det_offset[detector], stride, H,
                       (const int32_t*)res->order.p, (const int32_t*)res->n_root.p, (const int32_t*)res->d_root_cfg.p, (int32_t*)row_cfg.p);
    std::vector<int32_t> rcfg((size_t)H);
    HIP_TRY(hipMemcpyAsync(rcfg.data(), row_cfg.p, (size_t)H * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t h = 0; h < H; ++h) {
        const int32_t c = rcfg[(size_t)h];
        if (c < 0 || c >= K || (h > 0 && c < rcfg[(size_t)h - 1])) return fail(BMO_ERR_INTERNAL, refusal);
        if (R.count[(size_t)c]++ == 0) R.begin[(size_t)c] = h;
    }
    return BMO_OK;
}

// The splits of every configuration as one flat work list, and the launches that run it.
struct SplitPlan {
    struct Launch {
        int32_t c0, nc;  // configurations c0 .. c0 + nc - 1
        int64_t w0, nw;  // their work items
    };
    std::vector<int64_t> per_split;  // rows per split of every configuration
    std::vector<SplitCfg> cfg;
    std::vector<SplitWork> work;
    std::vector<Launch> launches;
    int64_t max_nw = 1;  // partial rows the largest launch writes

    // configuration c is split exactly as a single call with R.count[c] rows splits them; no launches (the spot read-outs run every item
    // in one launch)
    SplitPlan(const Ranges& R, unsigned pt_blocks, void (*splits)(int64_t, unsigned, int64_t&, int64_t&)) {
        const int32_t K = (int32_t)R.count.size();
        cfg.resize((size_t)K);
        per_split.assign((size_t)K, 0);
        for (int32_t c = 0; c < K; ++c) {
            cfg[(size_t)c] = SplitCfg{(int64_t)work.size(), 0, 0};
            const int64_t nh = R.count[(size_t)c];
            if (nh == 0) continue;
            int64_t ns, hps;
            splits(nh, pt_blocks, ns, hps);
            cfg[(size_t)c].n_splits = (int32_t)ns;
            per_split[(size_t)c] = hps;
            for (int64_t s = 0; s < ns; ++s) {
                const int64_t h0 = s * hps, h1 = h0 + hps < nh ? h0 + hps : nh;
                work.push_back(SplitWork{R.begin[(size_t)c] + h0, R.begin[(size_t)c] + h1, c, 0});
            }
        }
    }
    // the same with the launches of a read-out that writes n_pts partial sums per work item
    SplitPlan(const Ranges& R, unsigned pt_blocks, int64_t n_pts, void (*splits)(int64_t, unsigned, int64_t&, int64_t&)) : SplitPlan(R, pt_blocks, splits) {
        const int32_t K = (int32_t)R.count.size();
        // launches: consecutive configurations whose splits fit the grid's y limit and 1 GiB of partial sums (a configuration that alone
        // needs more goes alone; its split count is at most 65535)
        const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(65535, ((int64_t)1 << 30) / (n_pts * 16)));
        for (int32_t c = 0; c < K;) {
            Launch b{c, 0, cfg[(size_t)c].first_work, 0};
            while (c < K && b.nc < 65535 && (b.nc == 0 || b.nw + cfg[(size_t)c].n_splits <= cap)) b.nw += cfg[(size_t)c++].n_splits, ++b.nc;
            launches.push_back(b);
            max_nw = std::max(max_nw, b.nw);
        }
    }
};

// Runs the plan: accumulate(grid, launch, partial) queues the accumulate kernel of one launch, the reduction follows it.  `timer` is started
// here unless the caller's timing began earlier; kernel_ms is read from it once everything has run.
template <class Accumulate, class Finish>
static int split_reduce(const SplitPlan& plan, const SplitCfg* d_cfg, int64_t n_pts, hipStream_t st, EventTimer& timer, double* kernel_ms, Accumulate&& accumulate,
                        Finish finish) {
    DevBuf partial;
    if (int rc = partial.alloc((size_t)plan.max_nw * (size_t)n_pts * sizeof(double2))) return rc;
    if (!timer.e0)
        if (int rc = timer.start(st)) return rc;
    const unsigned pt_blocks = (unsigned)((n_pts + 255) / 256);
    for (const SplitPlan::Launch& b : plan.launches) {
        if (b.nw > 0) accumulate(dim3(pt_blocks, (unsigned)b.nw), b, (double2*)partial.p);
        hipLaunchKernelGGL(reduce_splits_kernel<Finish>, dim3(pt_blocks, (unsigned)b.nc), dim3(256), 0, st, d_cfg, b.c0, b.w0, (const double2*)partial.p, n_pts, finish);
    }
    return timer.stop(kernel_ms);
}

// the device and the device copy of the rows of a single call (d_rows holds an upload of host rows)
static int single_rows(const char* who, const double*& rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, int32_t device, DevBuf& d_rows) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BMO_ERR_NO_DEVICE, std::string(who) + ": no HIP device (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(BMO_ERR_INVALID, std::string(who) + ": bad device ordinal");
    HIP_TRY(hipSetDevice(device));
    if (!rows_on_device && n_rows > 0) {
        const size_t bytes = (size_t)n_rows * (size_t)row_cols * sizeof(double);
        if (int rc = d_rows.alloc(bytes)) return rc;
        HIP_TRY(hipMemcpy(d_rows.p, rows, bytes, hipMemcpyHostToDevice));
        rows = (const double*)d_rows.p;
    }
    return BMO_OK;
}

// What a read-out of resident rows checks of its result and slot before a device is touched: the slot exists and is a detector of `kind`
// (BMO_OBJ_SPOTDETECTOR or BMO_OBJ_PSFDETECTOR); with refuse_gaussian, the result is no GaussianBeamlet solution.  n_configs < 0: not checked.
static int slot_check(const char* who, const bmo_trace_result* res, int32_t detector, int32_t kind, bool refuse_gaussian, int32_t n_configs) {
    const bool spot = kind == BMO_OBJ_SPOTDETECTOR;
    if (detector < 0 || detector >= res->n_detectors) return fail(BMO_ERR_INVALID, std::string(who) + ": bad detector slot");
    if (refuse_gaussian && res->kind == BMO_BEAM_GAUSSIAN)
        return fail(BMO_ERR_UNSUPPORTED, std::string(who) + (spot ? ": a GaussianBeamlet solution has no Spotdetector rows (Spotdetector.jl:50 has no method for beamlets)"
                                                                  : ": a GaussianBeamlet solution has three rows per beamlet, not PSF rows"));
    if ((size_t)detector >= res->det_kind.size() || res->det_kind[(size_t)detector] != kind)
        return fail(BMO_ERR_INVALID, std::string(who) + (spot ? ": the slot is not a Spotdetector's" : ": the slot is not a PSFDetector's"));
    if (n_configs >= 0 && n_configs != std::max<int32_t>(res->n_configs, 1))
        return fail(BMO_ERR_INVALID, std::string(who) + ": n_configs must be the configuration count of the sweep result (1 for an ordinary result)");
    return BMO_OK;
}

// What the _sweep read-outs of resident rows end on, once the entry has made its checks and answered an empty slot: the result's device, the
// ranges of the slot's H > 0 rows over the n_configs configurations, and the rows themselves [H][9].
static int resident_rows(const char* who, bmo_trace_result* res, int32_t detector, int64_t H, int32_t n_configs, Ranges& R, const double*& rows) {
    HIP_TRY(hipSetDevice(res->device));
    const std::string refusal = std::string(who) + ": rows out of configuration order";
    if (int rc = slot_ranges(res, detector, 1, H, n_configs, res->n_configs > 0, refusal.c_str(), 0, R)) return rc;
    rows = (const double*)res->det_data.p + 9 * res->det_offset[detector];
    return BMO_OK;
}

// K rows of N columns as a configuration without rows reads: 0 in column 0 (the row count), NaN elsewhere
static void fill_empty_stats(double* out, size_t K, size_t N) {
    std::fill(out, out + K * N, std::nan(""));
    for (size_t c = 0; c < K; ++c) out[c * N] = 0.0;
}

// poses [K][3] as the kernels read them
static std::vector<PsfPose> psf_poses(size_t K, const double* origins, const double* e1s, const double* e2s) {
    std::vector<PsfPose> pose(K);
    for (size_t c = 0; c < K; ++c) {
        const double *o = origins + 3 * c, *a = e1s + 3 * c, *b = e2s + 3 * c;
        pose[c] = PsfPose{d3{o[0], o[1], o[2]}, d3{a[0], a[1], a[2]}, d3{b[0], b[1], b[2]}};
    }
    return pose;
}

// The PSF of the K = R.count.size() configurations from the device rows `hits`: poses [K][3], axes [K][n], outputs [K][n * n].
static int psf_read(const double* hits, const Ranges& R, const double* origins, const double* e1s, const double* e2s, const double* xs, const double* zs, int32_t n,
                    double* out_intensity, double* out_field, double* kernel_ms) {
    const size_t K = R.count.size();
    const int64_t n_pts = (int64_t)n * n;
    hipStream_t st = 0;
    const SplitPlan plan(R, (unsigned)((n_pts + 255) / 256), n_pts, psf_splits);
    const std::vector<PsfPose> pose = psf_poses(K, origins, e1s, e2s);
    Packed up;
    const size_t o_cfg = up.add(plan.cfg), o_work = up.add(plan.work), o_pose = up.add(pose), o_xs = up.add(xs, K * n), o_zs = up.add(zs, K * n);
    DevBuf d_int, d_field;
    int rc;
    if ((rc = up.upload(st)) || (rc = d_int.alloc(K * n_pts * sizeof(double))) || (out_field && (rc = d_field.alloc(K * n_pts * sizeof(double2))))) return rc;
    EventTimer timer;
    auto accumulate = [&](dim3 grid, const SplitPlan::Launch& L, double2* partial) {
        const size_t c = (size_t)L.c0;
        if (L.nc == 1)
            hipLaunchKernelGGL(psf_accumulate_kernel, grid, dim3(256), 0, st, hits + 9 * R.begin[c], R.count[c], plan.per_split[c], up.at<double>(o_xs) + c * n,
                               up.at<double>(o_zs) + c * n, n, pose[c].origin, pose[c].e1, pose[c].e2, partial);
        else
            hipLaunchKernelGGL(psf_accumulate_list_kernel, grid, dim3(256), 0, st, hits, up.at<SplitWork>(o_work), L.w0, up.at<PsfPose>(o_pose),
                               up.at<double>(o_xs), up.at<double>(o_zs), n, partial);
    };
    if ((rc = split_reduce(plan, up.at<SplitCfg>(o_cfg), n_pts, st, timer, kernel_ms, accumulate, PsfFinish{(double*)d_int.p, (double2*)d_field.p}))) return rc;
    HIP_TRY(hipMemcpy(out_intensity, d_int.p, K * n_pts * sizeof(double), hipMemcpyDeviceToHost));
    if (out_field) HIP_TRY(hipMemcpy(out_field, d_field.p, K * n_pts * sizeof(double2), hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_intensity(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                                 const double* xs, const double* zs, int32_t n, int32_t device, double* out_intensity, double* out_field, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !xs || !zs || !out_intensity || n <= 0 || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_intensity: bad argument");
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_intensity", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    return psf_read(hits, Ranges{{0}, {n_hits}}, origin, e1, e2, xs, zs, n, out_intensity, out_field, kernel_ms);
}

// PSF intensity of every configuration of a sweep, from the rows still resident in the result (an ordinary result is one configuration)
extern "C" int bmo_psf_intensity_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s,
                                       const double* e2s, const double* xs, const double* zs, int32_t n, double* out_intensity, double* out_field,
                                       double* kernel_ms) {
    if (!res || !origins || !e1s || !e2s || !xs || !zs || !out_intensity || n <= 0) return fail(BMO_ERR_INVALID, "bmo_psf_intensity_sweep: bad argument");
    if (int rc = slot_check("bmo_psf_intensity_sweep", res, detector, BMO_OBJ_PSFDETECTOR, false, n_configs)) return rc;  // Gaussian results are not refused here
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t n_pts = (int64_t)n * n;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_hits = 0
        std::fill(out_intensity, out_intensity + (size_t)n_configs * n_pts, 0.0);
        if (out_field) std::fill(out_field, out_field + (size_t)n_configs * n_pts * 2, 0.0);
        return BMO_OK;
    }
    Ranges R;
    const double* hits;
    if (int rc = resident_rows("bmo_psf_intensity_sweep", res, detector, H, n_configs, R, hits)) return rc;
    return psf_read(hits, R, origins, e1s, e2s, xs, zs, n, out_intensity, out_field, kernel_ms);
}

// ====================================================================================================================
// Photodetector field (Photodetector.jl:69-107).  Pipeline, all on the device the trace ran on:
//   1. pd_hit_nodes_kernel   : recorded beamlets of the slot (reference order) -> device node id, segment count, node->hit map
//   2. exclusive scan        : segment offsets of the per-hit segment table
//   3. pd_gather_kernel      : one pass over the step chunks of the segment log copies the chief / waist / divergence rays of
//                              those beamlets into a compact SoA table [24][total_segs] (+ the OPL carried in from the parent)
//   4. pd_prepare_kernel     : per beamlet, the hit-constant scalars in the reference's summation order: cumulative chief
//                              lengths (point_on_beam's `temp`), length(gauss), optical_path_length(gauss), l0, k, ref_phi
//   5. pd_field_kernel       : 256 grid points per workgroup x a contiguous range of beamlets; per pair the reference's
//                              expression sequence (point on the detector, projection on the beamlet axis, point_on_beam,
//                              gauss_parameters, electric_field); partial sums per beamlet range
//   6. reduce_splits_kernel  : sums the ranges in order and adds the result to the caller's field
// Steps 1 - 4 are pd_tables (bmo_gauss_parameters runs them for one beamlet), steps 5 - 6 the split-and-reduce pipeline above.
namespace {

enum { PD_SEG_PLANES = 24, PD_HS = 12 };
// per-hit scalars: 0 l_parent 1 w0 2 E0.re 3 E0.im 4 lambda 5 proj 6 opl_parent | prepared: 7 l0 8 k 9 ref_phi 10 len_total 11 unused

// Earlier segments of continued root beamlets (bmo_result_set_gauss_prefix): root node nd owns rows pre_start[nd] .. pre_start[nd + 1] of the
// prefix table; they come in front of the segments of the log.  nullptr: no beamlet has any.
struct PdPrefix {
    const int32_t* start;  // [n_roots + 1]
    const double* segs;    // [24][total]
    const double* opl;     // [n_roots]: optical path length of the parent chain
    int64_t n_roots, total;
    __device__ int len(int32_t nd) const { return (start && nd < n_roots) ? start[nd + 1] - start[nd] : 0; }
};


// Beamlet h of the tables is the one recorded on slot rows first_row + 3 h .. + 2 (row 0 = {proj, 0, ...}), or, with canon >= 0, the one
// beamlet is canonical node `canon` and proj = 1 (bmo_gauss_parameters).
__global__ void pd_hit_nodes_kernel(const int32_t* __restrict__ det_node, int64_t first_row, int64_t canon, int64_t n_hits, const int32_t* __restrict__ order,
                                    const int32_t* __restrict__ nseg, const double* __restrict__ aux, const double* __restrict__ lambda,
                                    const double* __restrict__ det_data, int32_t* __restrict__ hit_nseg, int32_t* __restrict__ node_hit,
                                    double* __restrict__ hs, PdPrefix pre) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_hits) return;
    const int64_t row = first_row + 3 * h;
    const int32_t nd = order[canon < 0 ? det_node[row] : canon];
    hit_nseg[h] = nseg[nd] + pre.len(nd);
    node_hit[nd] = (int32_t)h;
    double* s = hs + h * PD_HS;
    s[0] = aux[(int64_t)nd * 4 + 0];
    s[1] = aux[(int64_t)nd * 4 + 1];
    s[2] = aux[(int64_t)nd * 4 + 2];
    s[3] = aux[(int64_t)nd * 4 + 3];
    s[4] = lambda[nd];
    s[5] = canon < 0 ? det_data[row * 9 + 0] : 1.0;
}

__global__ void pd_gather_kernel(Chunk c, const int32_t* __restrict__ node_hit, const int32_t* __restrict__ seg_start, int64_t total_segs,
                                 double* __restrict__ segs, double* __restrict__ hs, PdPrefix pre) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.count) return;
    const int32_t nd = chunk_node(c, j);
    if (nd < 0) return;  // hole of a fused level
    const int32_t h = node_hit[nd];
    if (h < 0) return;
    const int32_t k = c.i[I_K * c.cap + j];
    const int plen = pre.len(nd);
    const int64_t dst = (int64_t)seg_start[h] + plen + k;
    for (int b = 0; b < 3; ++b)          // chief, waist, divergence: record planes 11*b + {pos 0-2, dir 3-5, n 6, t 7}
        for (int q = 0; q < 8; ++q) segs[(int64_t)(8 * b + q) * total_segs + dst] = c.d[(int64_t)(11 * b + q) * c.cap + j];
    if (k == 0) {
        // OPL of the parent chain (optical_path_length(parent)); a continued beamlet's record carries the OPL up to its open ray, the
        // parent's share of it came with the prefix
        hs[(int64_t)h * PD_HS + 6] = plen > 0 ? pre.opl[nd] : c.d[(int64_t)35 * c.cap + j];
        for (int i = 0; i < plen; ++i)
            for (int q = 0; q < PD_SEG_PLANES; ++q) segs[(int64_t)q * total_segs + seg_start[h] + i] = pre.segs[(int64_t)q * pre.total + pre.start[nd] + i];
    }
}

__global__ void pd_prepare_kernel(int64_t n_hits, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ hit_nseg, int64_t total_segs,
                                  const double* __restrict__ segs, double* __restrict__ cum, double* __restrict__ hs) {
    const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= n_hits) return;
    double* s = hs + h * PD_HS;
    const int64_t s0 = seg_start[h];
    const int ns = hit_nseg[h];
    const double* t = segs + 7 * total_segs;  // chief lengths
    const double* nn = segs + 6 * total_segs;  // chief refractive indices
    // point_on_beam (Beam.jl:177-205): temp = length(parent); temp += length(ray) for every ray but the last
    double temp = s[0];
    for (int k = 0; k + 1 < ns; ++k) {
        temp += t[s0 + k];
        cum[s0 + k] = temp;
    }
    cum[s0 + ns - 1] = kinf();
    // length(beam) = length_rays + length_parent (Beam.jl:125-130, :157-166); optical_path_length (Beam.jl:137-149)
    double l = 0.0, opl = s[6];
    for (int k = 0; k < ns; ++k) {
        l += t[s0 + k];
        opl += t[s0 + k] * nn[s0 + k];
    }
    const double len_total = l + s[0];
    s[10] = len_total;
    s[7] = len_total - t[s0 + ns - 1];                 // l0 = length(gauss) - length(ray)
    s[8] = 6.283185307179586 / s[4];                   // wave_number(λ) = 2π / λ
    s[9] = (opl - len_total) / s[4] * 6.283185307179586;  // ref_ϕ = Δl / λ * 2π
}

// point_on_beam(gauss.chief, z) (Beam.jl:177-205) on the compact segment table of beamlet h, and the chief / waist / divergence rays
// of the segment it selects: what gauss_parameters(gauss, z) (Gaussian.jl:298-353) starts from.
__device__ __forceinline__ RayS pd_ray_of(const double* __restrict__ segs, int64_t total_segs, int b, int64_t seg) {
    RayS r;
    const double* q = segs + (int64_t)(8 * b) * total_segs + seg;
    r.pos = {q[0], q[total_segs], q[2 * total_segs]};
    r.dir = {q[3 * total_segs], q[4 * total_segs], q[5 * total_segs]};
    r.n = q[6 * total_segs];
    return r;
}
__device__ __forceinline__ void pd_locate(double z, int64_t s0, int ns, double l_parent, const double* __restrict__ segs, const double* __restrict__ cum,
                                          int64_t total_segs, const RayS& c_last, RayS& cr, RayS& wr, RayS& dr, d3& p0) {
    const int64_t last = s0 + ns - 1;
    int64_t seg = last;
    if (ns > 1 && z < cum[last - 1]) {  // first ray (but the last) whose cumulative length exceeds z
        seg = s0;
        while (!(z < cum[seg])) ++seg;  // terminates: z < cum[last - 1]
        const double len = segs[7 * total_segs + seg];
        const double bb = cum[seg] - z;
        const RayS c = pd_ray_of(segs, total_segs, 0, seg);
        p0 = axpy3(c.pos, len - bb, c.dir);
    } else {
        const double temp = ns > 1 ? cum[last - 1] : l_parent;
        p0 = axpy3(c_last.pos, z - temp, c_last.dir);
    }
    cr = seg == last ? c_last : pd_ray_of(segs, total_segs, 0, seg);
    wr = pd_ray_of(segs, total_segs, 1, seg);
    dr = pd_ray_of(segs, total_segs, 2, seg);
}

struct PdGeom {
    double p[3];   // position(shape(pd))
    double ox[3];  // T[k,1] = orientation[1,k]: the x step in world coordinates (Photodetector.jl:76, :91-95)
    double oy[3];  // T[k,3] = orientation[3,k]
};

// The field of beamlets h0 .. h1 - 1 at detector point p1, summed in beamlet order (the blocked order of bmo_photodetector_field: one range
// per workgroup row, the ranges summed by reduce_splits_kernel)
__device__ __forceinline__ double2 pd_field_range(const d3& p1, int64_t h0, int64_t h1, const int32_t* __restrict__ seg_start, const int32_t* __restrict__ hit_nseg,
                                                  int64_t total_segs, const double* __restrict__ segs, const double* __restrict__ cum, const double* __restrict__ hs) {
    double fre = 0.0, fim = 0.0;
    for (int64_t h = h0; h < h1; ++h) {  // wave-uniform: every lane walks the same beamlets (broadcast loads)
        const double* s = hs + h * PD_HS;
        const int64_t s0 = seg_start[h];
        const int ns = hit_nseg[h];
        const int64_t last = s0 + ns - 1;
        const RayS c_last = pd_ray_of(segs, total_segs, 0, last);
        // projection of the detector point on the optical axis of the last chief ray
        const d3 dp = sub3(p1, c_last.pos);
        const double l1 = dot3(dp, c_last.dir);
        const d3 p2 = axpy3(c_last.pos, l1, c_last.dir);
        const double r = norm3(sub3(p1, p2));
        const double z = s[7] + l1;
        RayS cr, wr, dr;
        d3 p0;
        pd_locate(z, s0, ns, s[0], segs, cum, total_segs, c_last, cr, wr, dr, p0);
        double w, R, psi, w0;
        gauss_parameters_at(cr, wr, dr, p0, s[4], w, R, psi, w0);
        // electric_field(gauss, r, z) Gaussian.jl:381-392
        const double ratio = s[1] / w0;                                  // beam_waist(gauss) / w0
        cx E{s[2] * ratio, s[3] * ratio};                                // E0 = electric_field(gauss) * ratio
        const double kk = s[8];
        // electric_field(r, z, E0, w0, w, k, ψ, R) OpticUtils.jl:87-89: E0 * w0 / w * exp(-r^2 / w^2) * exp(im * (k*z + ψ + (k*r^2*R)/2))
        E = cx{E.re * w0, E.im * w0};
        E = cx{E.re / w, E.im / w};
        const double ga = exp(-(r * r) / (w * w));
        E = cx{E.re * ga, E.im * ga};
        const double ph = kk * z + psi + (kk * (r * r) * R) / 2;
        double sn, cs;
        sincos(ph, &sn, &cs);
        E = cmul(E, cx{cs, sn});
        sincos(s[9], &sn, &cs);                                          // * exp(im * ref_ϕ)
        E = cmul(E, cx{cs, sn});
        const double sp = sqrt(s[5]);                                    // * sqrt(proj)
        fre += E.re * sp;
        fim += E.im * sp;
    }
    return make_double2(fre, fim);
}

// work item w0 + blockIdx.y at the points of its configuration's detector pose
__global__ __launch_bounds__(256) void pd_field_kernel(const SplitWork* __restrict__ work, int64_t w0, const PdGeom* __restrict__ geom,
                                                       const int32_t* __restrict__ seg_start, const int32_t* __restrict__ hit_nseg, int64_t total_segs,
                                                       const double* __restrict__ segs, const double* __restrict__ cum, const double* __restrict__ hs,
                                                       const double* __restrict__ xs, const double* __restrict__ ys, int32_t nx, int32_t ny,
                                                       double2* __restrict__ partial) {
    const int64_t n_pts = (int64_t)nx * ny;
    const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pt >= n_pts) return;
    const SplitWork W = work[w0 + blockIdx.y];
    const PdGeom& G = geom[W.cfg];
    const int i = (int)(pt % nx), j = (int)(pt / nx);
    const double x = xs[i], y = ys[j];
    const d3 p1{G.ox[0] * x + G.oy[0] * y + G.p[0], G.ox[1] * x + G.oy[1] * y + G.p[1], G.ox[2] * x + G.oy[2] * y + G.p[2]};
    partial[(int64_t)blockIdx.y * n_pts + pt] = pd_field_range(p1, W.h0, W.h1, seg_start, hit_nseg, total_segs, segs, cum, hs);
}

// gauss_parameters(gauss, z) for the one beamlet of the tables at n values of z: the same locate / gauss_parameters_at sequence the
// Photodetector field runs per grid point
__global__ void gp_eval_kernel(int32_t n, const double* __restrict__ zs, int ns, int64_t total_segs, const double* __restrict__ segs, const double* __restrict__ cum,
                               const double* __restrict__ hs, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RayS c_last = pd_ray_of(segs, total_segs, 0, ns - 1);
    RayS cr, wr, dr;
    d3 p0;
    pd_locate(zs[i], 0, ns, hs[0], segs, cum, total_segs, c_last, cr, wr, dr, p0);
    double w, R, psi, w0;
    gauss_parameters_at(cr, wr, dr, p0, hs[4], w, R, psi, w0);
    out[4 * i + 0] = w;
    out[4 * i + 1] = R;
    out[4 * i + 2] = psi;
    out[4 * i + 3] = w0;
}

}  // namespace

static PdPrefix prefix_of(const bmo_trace_result* res) {
    PdPrefix p{nullptr, nullptr, nullptr, 0, 0};
    if (res->pre_start.p) p = PdPrefix{(const int32_t*)res->pre_start.p, (const double*)res->pre_segs.p, (const double*)res->pre_opl.p, res->pre_roots, res->pre_total};
    return p;
}

extern "C" int bmo_result_set_gauss_prefix(bmo_trace_result* res, int64_t n_roots, const int32_t* prefix_start, const double* prefix_segs, const double* opl_parent) {
    if (!res || !prefix_start || !opl_parent || n_roots <= 0) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: bad argument");
    if (res->kind != BMO_BEAM_GAUSSIAN) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: not a GaussianBeamlet solution");
    if (n_roots != res->n_roots) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: one entry per root beamlet of the solution is expected");
    if (prefix_start[0] != 0) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: prefix_start[0] must be 0");
    for (int64_t i = 0; i < n_roots; ++i)
        if (prefix_start[i + 1] < prefix_start[i]) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: prefix_start must not decrease");
    const int64_t total = prefix_start[n_roots];
    if (total > 0 && !prefix_segs) return fail(BMO_ERR_INVALID, "bmo_result_set_gauss_prefix: prefix_segs missing");
    HIP_TRY(hipSetDevice(res->device));
    int rc;
    res->pre_start.release();
    res->pre_segs.release();
    res->pre_opl.release();
    if ((rc = res->pre_start.alloc((size_t)(n_roots + 1) * 4)) || (rc = res->pre_segs.alloc((size_t)std::max<int64_t>(total, 1) * PD_SEG_PLANES * 8)) ||
        (rc = res->pre_opl.alloc((size_t)n_roots * 8)))
        return rc;
    HIP_TRY(hipMemcpy(res->pre_start.p, prefix_start, (size_t)(n_roots + 1) * 4, hipMemcpyHostToDevice));
    if (total > 0) HIP_TRY(hipMemcpy(res->pre_segs.p, prefix_segs, (size_t)total * PD_SEG_PLANES * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(res->pre_opl.p, opl_parent, (size_t)n_roots * 8, hipMemcpyHostToDevice));
    res->pre_roots = n_roots;
    res->pre_total = total;
    return BMO_OK;
}

// Steps 1 - 4 of the Photodetector pipeline for H beamlets (pd_hit_nodes_kernel: slot rows from first_row, or node `canon`): the compact
// segment table and the per-beamlet scalars.
struct PdTables {
    DevBuf hit_nseg, node_hit, seg_start, hs, tmp, segs, cum;
    int64_t total_segs = 0;
};
static int pd_tables(bmo_trace_result* res, int64_t first_row, int64_t canon, int64_t H, hipStream_t st, const char* who, PdTables& T) {
    const int64_t nn = res->n_nodes;
    int rc;
    if ((rc = T.hit_nseg.alloc((size_t)H * 4)) || (rc = T.node_hit.alloc((size_t)nn * 4)) || (rc = T.seg_start.alloc((size_t)H * 4)) ||
        (rc = T.hs.alloc((size_t)H * PD_HS * 8)))
        return rc;
    HIP_TRY(hipMemsetAsync(T.node_hit.p, 0xFF, (size_t)nn * 4, st));
    HIP_TRY(hipMemsetAsync(T.hs.p, 0, (size_t)H * PD_HS * 8, st));
    const unsigned hb = (unsigned)((H + 255) / 256);
    hipLaunchKernelGGL(pd_hit_nodes_kernel, dim3(hb), dim3(256), 0, st, (const int32_t*)res->det_node.p, first_row, canon, H, (const int32_t*)res->order.p,
                       (const int32_t*)res->n_nseg.p, (const double*)res->n_aux.p, (const double*)res->n_lambda.p, (const double*)res->det_data.p,
                       (int32_t*)T.hit_nseg.p, (int32_t*)T.node_hit.p, (double*)T.hs.p, prefix_of(res));
    CUB_TRY(scratch_in(T.tmp), hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)T.hit_nseg.p, (int32_t*)T.seg_start.p, (int)H, st));
    int32_t last_start = 0, last_n = 0;
    HIP_TRY(hipMemcpyAsync(&last_start, (const int32_t*)T.seg_start.p + H - 1, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_n, (const int32_t*)T.hit_nseg.p + H - 1, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    T.total_segs = (int64_t)last_start + last_n;
    if (T.total_segs <= 0) return fail(BMO_ERR_INTERNAL, std::string(who) + ": beamlet without segments");
    if ((rc = T.segs.alloc((size_t)T.total_segs * PD_SEG_PLANES * 8)) || (rc = T.cum.alloc((size_t)T.total_segs * 8))) return rc;
    for (const Chunk& c : res->chunks)
        if (c.count > 0)
            hipLaunchKernelGGL(pd_gather_kernel, dim3((unsigned)((c.count + 255) / 256)), dim3(256), 0, st, c, (const int32_t*)T.node_hit.p,
                               (const int32_t*)T.seg_start.p, T.total_segs, (double*)T.segs.p, (double*)T.hs.p, prefix_of(res));
    hipLaunchKernelGGL(pd_prepare_kernel, dim3(hb), dim3(256), 0, st, H, (const int32_t*)T.seg_start.p, (const int32_t*)T.hit_nseg.p, T.total_segs,
                       (const double*)T.segs.p, (double*)T.cum.p, (double*)T.hs.p);
    return BMO_OK;
}

extern "C" int bmo_gauss_parameters(bmo_trace_result* res, int64_t node, const double* zs, int32_t n, double* out) {
    if (!res || !zs || !out || n <= 0) return fail(BMO_ERR_INVALID, "bmo_gauss_parameters: bad argument");
    if (res->kind != BMO_BEAM_GAUSSIAN) return fail(BMO_ERR_INVALID, "bmo_gauss_parameters: not a GaussianBeamlet solution");
    if (node < 0 || node >= res->n_nodes) return fail(BMO_ERR_INVALID, "bmo_gauss_parameters: bad beamlet index");
    if (!res->has_log) return fail(BMO_ERR_INVALID, "bmo_gauss_parameters: the solution was solved with record_segments = 0 (no segments to evaluate)");
    HIP_TRY(hipSetDevice(res->device));
    int rc;
    PdTables T;
    DevBuf d_z, d_out;
    hipStream_t st = 0;
    if ((rc = pd_tables(res, 0, node, 1, st, "bmo_gauss_parameters", T)) || (rc = d_z.alloc((size_t)n * 8)) || (rc = d_out.alloc((size_t)n * 32))) return rc;
    HIP_TRY(hipMemcpyAsync(d_z.p, zs, (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gp_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const double*)d_z.p, (int)T.total_segs, T.total_segs,
                       (const double*)T.segs.p, (const double*)T.cum.p, (const double*)T.hs.p, (double*)d_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out.p, (size_t)n * 32, hipMemcpyDeviceToHost));
    return BMO_OK;
}

static PdGeom pd_geom(const double position[3], const double orientation[9]) {
    PdGeom G;
    for (int k = 0; k < 3; ++k) {
        G.p[k] = position[k];
        G.ox[k] = orientation[0 * 3 + k];  // T[k,1] with T = transpose(orientation)
        G.oy[k] = orientation[2 * 3 + k];  // T[k,3]
    }
    return G;
}

// The field of the H beamlets of the slot added to field_inout [K][nx * ny], configuration c at pose c (positions [K][3], orientations
// [K][9]).  order_refusal: the result is a sweep's and every beamlet counts for its own configuration; nullptr: one configuration has all.
// kernel_ms covers everything on the device, the tables included.
static int pd_read(bmo_trace_result* res, int32_t detector, int64_t H, int32_t K, const char* who, const char* order_refusal, const double* positions,
                   const double* orientations, const double* xs, const double* ys, int32_t nx, int32_t ny, double* field_inout, double* kernel_ms) {
    HIP_TRY(hipSetDevice(res->device));
    const int64_t n_pts = (int64_t)nx * ny;
    const size_t field_bytes = (size_t)K * n_pts * sizeof(double2);
    hipStream_t st = 0;
    int rc;
    PdTables T;
    Ranges R;
    EventTimer timer;
    if ((rc = timer.start(st)) || (rc = pd_tables(res, res->det_offset[detector], -1, H, st, who, T)) ||
        (rc = slot_ranges(res, detector, 3, H, K, order_refusal != nullptr, order_refusal, st, R)))
        return rc;
    const SplitPlan plan(R, (unsigned)((n_pts + 255) / 256), n_pts, pd_splits);
    std::vector<PdGeom> geom((size_t)K);
    for (size_t c = 0; c < (size_t)K; ++c) geom[c] = pd_geom(positions + 3 * c, orientations + 9 * c);
    Packed up;
    const size_t o_cfg = up.add(plan.cfg), o_work = up.add(plan.work), o_geom = up.add(geom), o_xs = up.add(xs, (size_t)nx), o_ys = up.add(ys, (size_t)ny);
    DevBuf d_field;
    if ((rc = up.upload(st)) || (rc = d_field.alloc(field_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(d_field.p, field_inout, field_bytes, hipMemcpyHostToDevice, st));
    auto accumulate = [&](dim3 grid, const SplitPlan::Launch& L, double2* partial) {
        hipLaunchKernelGGL(pd_field_kernel, grid, dim3(256), 0, st, up.at<SplitWork>(o_work), L.w0, up.at<PdGeom>(o_geom), (const int32_t*)T.seg_start.p,
                           (const int32_t*)T.hit_nseg.p, T.total_segs, (const double*)T.segs.p, (const double*)T.cum.p, (const double*)T.hs.p,
                           up.at<double>(o_xs), up.at<double>(o_ys), nx, ny, partial);
    };
    if ((rc = split_reduce(plan, up.at<SplitCfg>(o_cfg), n_pts, st, timer, kernel_ms, accumulate, PdFinish{(double2*)d_field.p}))) return rc;
    HIP_TRY(hipMemcpy(field_inout, d_field.p, field_bytes, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_photodetector_field(bmo_trace_result* res, int32_t detector, const double position[3], const double orientation[9], const double* xs,
                                       const double* ys, int32_t nx, int32_t ny, double* field_inout, double* kernel_ms) {
    if (!res || !position || !orientation || !xs || !ys || !field_inout || nx <= 0 || ny <= 0) return fail(BMO_ERR_INVALID, "bmo_photodetector_field: bad argument");
    if (detector < 0 || detector >= res->n_detectors) return fail(BMO_ERR_INVALID, "bmo_photodetector_field: bad detector slot");
    if (kernel_ms) *kernel_ms = 0.0;
    if (res->kind != BMO_BEAM_GAUSSIAN) return BMO_OK;  // other beams leave no record (Photodetector.jl:57-60)
    const int64_t rows = res->det_count[detector];
    if (rows % 3) return fail(BMO_ERR_INVALID, "bmo_photodetector_field: slot does not hold photodetector records");
    if (rows == 0) return BMO_OK;
    if (!res->has_log) return fail(BMO_ERR_INVALID, "bmo_photodetector_field: the solution was solved with record_segments = 0 (gauss_parameters needs the beamlets' segments)");
    return pd_read(res, detector, rows / 3, 1, "bmo_photodetector_field", nullptr, position, orientation, xs, ys, nx, ny, field_inout, kernel_ms);
}

extern "C" int bmo_photodetector_field_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* positions, const double* orientations,
                                             const double* xs, const double* ys, int32_t nx, int32_t ny, double* field_inout, double* kernel_ms) {
    if (!res || !positions || !orientations || !xs || !ys || !field_inout || nx <= 0 || ny <= 0)
        return fail(BMO_ERR_INVALID, "bmo_photodetector_field_sweep: bad argument");
    if (detector < 0 || detector >= res->n_detectors) return fail(BMO_ERR_INVALID, "bmo_photodetector_field_sweep: bad detector slot");
    if (res->n_configs < 1 || n_configs != res->n_configs)
        return fail(BMO_ERR_INVALID, "bmo_photodetector_field_sweep: n_configs must be the configuration count of the sweep result");
    if (kernel_ms) *kernel_ms = 0.0;
    if (res->kind != BMO_BEAM_GAUSSIAN) return BMO_OK;  // other beams leave no record (Photodetector.jl:57-60)
    const int64_t rows = res->det_count[detector];
    if (rows % 3) return fail(BMO_ERR_INVALID, "bmo_photodetector_field_sweep: slot does not hold photodetector records");
    if (rows == 0) return BMO_OK;
    if (!res->has_log) return fail(BMO_ERR_INVALID, "bmo_photodetector_field_sweep: the solution was solved with record_segments = 0 (gauss_parameters needs the beamlets' segments)");
    return pd_read(res, detector, rows / 3, n_configs, "bmo_photodetector_field_sweep", "bmo_photodetector_field_sweep: beamlets out of configuration order", positions,
                   orientations, xs, ys, nx, ny, field_inout, kernel_ms);
}

// ====================================================================================================================
// Spot read-out: the binned image and the moment statistics of a Spotdetector's rows (include/bmo.h "Spot read-out").  The rows are
// [n][cols] doubles with x in column 0 and z in column 1: the packed columns of bmo_result_copy_hit_columns, or the resident 9-column rows
// of a slot (a 72-byte stride of which 16 bytes are used; every lane reads its own row with vector loads).  The same plumbing as above:
//   * slot_ranges gives the rows of every configuration, SplitPlan cuts each into splits (spot_splits: multiples of 256 rows) and lists
//     them as flat work items.  The items lie on the grid's x dimension (limit 2^31 - 1), so one launch runs them all (SplitPlan's
//     constructor without launches).  A single call is the K = 1 case, and configuration c is split exactly as a single call with its rows.
//   * image: one workgroup per item bins its rows into a privatised uint32 histogram in LDS (images of up to SPOT_LDS_BINS bins), then adds
//     the non-zero bins to image[c] with 64-bit global atomics; larger images are added to global memory directly.  Counts are integers:
//     the result does not depend on the order of the adds.  Lanes of a wave that hit the same bin are counted by one of them (spot_add).
//   * statistics: two accumulate kernels with a per-configuration reduce each, queued behind one synchronisation; the centroid stays on
//     the device for the second pass.  Lane l of a workgroup sums rows h0 + l, h0 + l + 256, ... sequentially, a fixed tree runs over the
//     lanes of a wave and the four waves, the splits are summed in split order: deterministic for a given row count.  The sums of a pass
//     are a sum record (below), which the wavefront, Zernike and focus statistics share with this read-out, as they do the walk over a
//     work item's rows (sum_pass_strided, sum_pass_staged), the host side of the passes (RowPasses) and single_rows.
namespace {

constexpr int SPOT_MIN_SPLIT = 2048;   // rows: shorter splits would spend their time on the histogram, not on rows
constexpr int SPOT_MAX_SPLITS = 2048;  // per configuration: eight workgroups per CU
constexpr int SPOT_LDS_BINS = 16384;   // uint32 counters in 64 KB of LDS
constexpr int SPOT_AGG_ITERS = 4;      // distinct bins a wave counts by ballot before the remaining lanes add one by one (0: plain atomics)

struct SpotWindow {
    double x0, x1, z0, z1, sx, sz;  // sx = nx / (x1 - x0), sz = nz / (z1 - z0)
};

// the binning rule: bin i + nx * j of (x, z), -1 outside (plain compares: a NaN is outside, the upper edge is closed)
__device__ __forceinline__ int32_t spot_bin(double x, double z, const SpotWindow& W, int32_t nx, int32_t nz) {
    if (!(x >= W.x0 && x <= W.x1 && z >= W.z0 && z <= W.z1)) return -1;
    int64_t i = (int64_t)floor((x - W.x0) * W.sx), j = (int64_t)floor((z - W.z0) * W.sz);
    if (i > nx - 1) i = nx - 1;
    if (j > nz - 1) j = nz - 1;
    return (int32_t)(i + (int64_t)nx * j);
}

// hist[key] += 1 for every lane with `live`.  A focused spot puts all 64 lanes on one bin: the first live lane takes its bin, the lanes
// that share it are counted by ballot and it adds their number; after SPOT_AGG_ITERS such bins the lanes left add one each.  Called by
// whole waves (a lane without a row passes live = false).
template <class Counter>
__device__ __forceinline__ void spot_add(Counter* hist, int32_t key, bool live) {
    const int lane = (int)(threadIdx.x & 63);
    for (int it = 0; it < SPOT_AGG_ITERS; ++it) {
        if (live) {
            const int32_t k = __builtin_amdgcn_readfirstlane(key);
            const unsigned long long m = __ballot(key == k);
            if (lane == __ffsll((long long)m) - 1) atomicAdd(&hist[k], (Counter)__popcll(m));
            if (key == k) live = false;
        }
    }
    if (live) atomicAdd(&hist[key], (Counter)1);
}

// work item blockIdx.x: its rows binned into image[cfg], the rows outside the window counted in outside[cfg]
template <bool LDS>
__global__ __launch_bounds__(256) void spot_image_kernel(const double* __restrict__ rows, int32_t cols, const SplitWork* __restrict__ work,
                                                         const SpotWindow* __restrict__ win, int32_t nx, int32_t nz, unsigned long long* __restrict__ image,
                                                         unsigned long long* __restrict__ outside) {
    extern __shared__ uint32_t spot_hist[];  // LDS: nx * nz counters
    const SplitWork W = work[blockIdx.x];
    const SpotWindow B = win[W.cfg];
    const int32_t n_bins = nx * nz;
    unsigned long long* img = image + (int64_t)W.cfg * n_bins;
    if (LDS) {
        for (int32_t b = threadIdx.x; b < n_bins; b += 256) spot_hist[b] = 0;
        __syncthreads();
    }
    uint32_t n_out = 0;
    for (int64_t base = W.h0; base < W.h1; base += 256) {  // workgroup-uniform trips: spot_add needs whole waves
        const int64_t h = base + threadIdx.x;
        int32_t key = -1;
        if (h < W.h1) {
            const double* r = rows + h * cols;
            key = spot_bin(r[0], r[1], B, nx, nz);
            n_out += key < 0;
        }
        if (LDS) spot_add(spot_hist, key, key >= 0);
        else spot_add(img, key, key >= 0);
    }
    for (int off = 32; off > 0; off >>= 1) n_out += __shfl_down(n_out, off);
    if ((threadIdx.x & 63) == 0 && n_out) atomicAdd(&outside[W.cfg], (unsigned long long)n_out);
    if (LDS) {
        __syncthreads();
        for (int32_t b = threadIdx.x; b < n_bins; b += 256) {
            const uint32_t v = spot_hist[b];
            if (v) atomicAdd(&img[b], (unsigned long long)v);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------------
// Sum records: what the statistics passes of the spot, wavefront, Zernike and focus read-outs share.  A pass keeps a few running sums,
// minima and maxima.  SUM_RECORD declares them once, as a list F(name, operation); the record has one double per field, and the identity,
// the merge of two partial results, the reduction over the workgroup and the fold of a configuration's work items all come from that list.
// An accumulate kernel starts every lane from sum_identity, updates the named fields with its own arithmetic and writes sum_wg_reduce of
// the record, one per work item; sum_reduce_kernel folds the work items of a configuration in split order and hands the result to a Finish.
struct SumAdd {
    static __device__ double identity() { return 0.0; }
    __device__ double operator()(double a, double b) const { return a + b; }
};
struct SumMin {
    static __device__ double identity() { return kinf(); }
    __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};
struct SumMax {
    static __device__ double identity() { return -kinf(); }
    __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};
// the maximum of a quantity that is never negative (a half-width, a squared radius): it starts at 0, so rows that compare false (NaN)
// leave 0 and not -inf
struct SumMax0 : SumMax {
    static __device__ double identity() { return 0.0; }
};

#define SUM_FIELD_DECL(name, Op) double name;
#define SUM_FIELD_COUNT(name, Op) +1
#define SUM_FIELD_VISIT(name, Op) f(a.name, b.name, Op{});
#define SUM_RECORD(Name, FIELDS)                                                                         \
    struct Name {                                                                                        \
        FIELDS(SUM_FIELD_DECL)                                                                           \
        static constexpr int N = 0 FIELDS(SUM_FIELD_COUNT);                                              \
        /* f(field of a, field of b, the field's operation) for every field in the order of the list */  \
        template <class A, class B, class F>                                                             \
        static __device__ __forceinline__ void visit(A& a, B& b, F&& f) {                                \
            FIELDS(SUM_FIELD_VISIT)                                                                      \
        }                                                                                                \
    };                                                                                                   \
    static_assert(sizeof(Name) == Name::N * sizeof(double), "a sum record is its fields")

template <class R>
__device__ __forceinline__ R sum_identity() {
    R r;
    R::visit(r, r, [](double& v, const double&, auto op) { v = op.identity(); });
    return r;
}
// acc and other merged field by field, the accumulator on the left
template <class R>
__device__ __forceinline__ void sum_merge(R& acc, const R& other) {
    R::visit(acc, other, [](double& a, const double& b, auto op) { a = op(a, b); });
}
// The records of the workgroup's 256 lanes merged by a fixed tree per field: over the lanes of a wave, then (w0 + w1) + (w2 + w3).  Thread 0
// returns the result.  Every lane calls it (it syncs); all fields cross LDS between one pair of barriers.
template <class R>
__device__ __forceinline__ R sum_wg_reduce(R r) {
    __shared__ double sh[R::N][4];
    R::visit(r, r, [](double& v, const double&, auto op) {
        for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_down(v, off));
    });
    __syncthreads();  // sh is free again
    if ((threadIdx.x & 63) == 0) {
        int q = 0;
        R::visit(r, r, [&](double& v, const double&, auto) { sh[q++][threadIdx.x >> 6] = v; });
    }
    __syncthreads();
    int q = 0;
    R::visit(r, r, [&](double& v, const double&, auto op) {
        v = op(op(sh[q][0], sh[q][1]), op(sh[q][2], sh[q][3]));
        ++q;
    });
    return r;
}

// The records first .. first + n - 1 folded in that order by thread 0 of the workgroup, which returns the result.  A configuration of 2 048
// splits would keep one thread waiting on 2 048 dependent trips to memory; instead the workgroup copies them to `lds` with coalesced loads,
// SUM_FOLD_CHUNK at a time, and thread 0 folds them from there.  Every thread of the workgroup calls it (it syncs).
constexpr int SUM_FOLD_CHUNK = 512;
template <class R>
__device__ __forceinline__ R sum_fold(const R* __restrict__ partial, int64_t first, int n, double* lds) {
    R acc = sum_identity<R>();
    for (int s0 = 0; s0 < n; s0 += SUM_FOLD_CHUNK) {
        const int cnt = n - s0 < SUM_FOLD_CHUNK ? n - s0 : SUM_FOLD_CHUNK;
        const double* src = (const double*)(partial + first + s0);
        __syncthreads();
        for (int q = threadIdx.x; q < cnt * R::N; q += blockDim.x) lds[q] = src[q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < cnt; ++i) sum_merge(acc, *(const R*)(lds + i * R::N));
    }
    return acc;
}

// Range blockIdx.x of `cfg` (a configuration, or a plane of the focus statistics): its records folded in split order, then thread 0 calls
// finish(blockIdx.x, record), or finish.empty(blockIdx.x) for a range without records.  The functor owns what the passes differ in: what
// goes to the caller's statistics and what stays on the device for the next pass.
template <class R, class Finish>
__global__ void sum_reduce_kernel(const SplitCfg* __restrict__ cfg, const R* __restrict__ partial, Finish finish) {
    __shared__ double lds[SUM_FOLD_CHUNK * R::N];
    const int32_t c = (int32_t)blockIdx.x;
    const SplitCfg C = cfg[c];
    if (C.n_splits == 0) {
        if (threadIdx.x == 0) finish.empty(c);
        return;
    }
    const R r = sum_fold(partial, C.first_work, C.n_splits, lds);
    if (threadIdx.x == 0) finish(c, r);
}
// the reduce of the n ranges of `cfg` over the records R of `partial`: one workgroup per range
template <class R, class Finish>
static void sum_reduce(unsigned n, hipStream_t st, const SplitCfg* cfg, const DevBuf& partial, Finish finish) {
    hipLaunchKernelGGL((sum_reduce_kernel<R, Finish>), dim3(n), dim3(256), 0, st, cfg, (const R*)partial.p, finish);
}

// How a statistics pass walks the rows W.h0 .. W.h1 - 1 of its work item, written once; the kernels are their bodies.
// Tile-staged, for passes that use all nine columns: tiles of PSF_TILE rows go through LDS with coalesced loads (psf_stage_rows) and lane l
// then reads row l of the tile (a 72-byte stride: the lanes of a half-wave fall on distinct even banks).  body(r, h): r the staged row, h
// its index.  Every lane of the workgroup calls it (it syncs).
template <class Body>
__device__ __forceinline__ void rows_staged(const double* __restrict__ hits, const SplitWork& W, Body&& body) {
    __shared__ double tile[PSF_TILE * 9];
    for (int64_t base = W.h0; base < W.h1; base += PSF_TILE) {
        const int cnt = (int)(W.h1 - base < PSF_TILE ? W.h1 - base : PSF_TILE);
        psf_stage_rows(hits, base, cnt, tile);
        if ((int)threadIdx.x < cnt) body(tile + 9 * threadIdx.x, base + threadIdx.x);
    }
}
// A pass of work item blockIdx.x that keeps one record per lane: every lane starts from the identity, the body adds the lane's rows in the
// order of the walk, the workgroup's record goes to partial[blockIdx.x].  Staged: body(record, r, h).
template <class R, class Body>
__device__ __forceinline__ void sum_pass_staged(const double* __restrict__ hits, const SplitWork& W, R* __restrict__ partial, Body&& body) {
    R a = sum_identity<R>();
    rows_staged(hits, W, [&](const double* r, int64_t h) { body(a, r, h); });
    a = sum_wg_reduce(a);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}
// Strided, for passes that read a few columns straight from memory: lane l visits rows h0 + l, h0 + l + 256, ...; body(record, h).
template <class R, class Body>
__device__ __forceinline__ void sum_pass_strided(const SplitWork& W, R* __restrict__ partial, Body&& body) {
    R a = sum_identity<R>();
    for (int64_t h = W.h0 + threadIdx.x; h < W.h1; h += 256) body(a, h);
    a = sum_wg_reduce(a);
    if (threadIdx.x == 0) partial[blockIdx.x] = a;
}

// --------------------------------------------------------------------------------------------------------------------
// Spot statistics
#define SPOT_SUM1(F) F(sx, SumAdd) F(sz, SumAdd) F(x_min, SumMin) F(x_max, SumMax) F(z_min, SumMin) F(z_max, SumMax)
#define SPOT_SUM2(F) F(xx, SumAdd) F(zz, SumAdd) F(xz, SumAdd) F(r2, SumMax0)
SUM_RECORD(SpotSum1, SPOT_SUM1);
SUM_RECORD(SpotSum2, SPOT_SUM2);

// first pass of work item blockIdx.x: sums and extrema of its rows
__global__ __launch_bounds__(256) void spot_centroid_kernel(const double* __restrict__ rows, int32_t cols, const SplitWork* __restrict__ work,
                                                            SpotSum1* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    sum_pass_strided(W, partial, [&](SpotSum1& a, int64_t h) {
        const double* r = rows + h * cols;
        const double x = r[0], z = r[1];
        a.sx += x;
        a.sz += z;
        a.x_min = x < a.x_min ? x : a.x_min;
        a.x_max = x > a.x_max ? x : a.x_max;
        a.z_min = z < a.z_min ? z : a.z_min;
        a.z_max = z > a.z_max ? z : a.z_max;
    });
}

// N, the centroid and the extrema go to stats[c], the centroid to cent[c] for the second pass
struct SpotCentroidFinish {
    const int64_t* count;
    double* stats;
    double2* cent;
    __device__ void empty(int32_t c) const {
        double* out = stats + (int64_t)c * BMO_SPOT_STAT_N;
        out[BMO_SPOT_STAT_N_ROWS] = 0.0;
        for (int q = 1; q < BMO_SPOT_STAT_N; ++q) out[q] = knan();
        cent[c] = make_double2(0.0, 0.0);
    }
    __device__ void operator()(int32_t c, const SpotSum1& s) const {
        double* out = stats + (int64_t)c * BMO_SPOT_STAT_N;
        const int64_t n = count[c];
        const double cx = s.sx / (double)n, cz = s.sz / (double)n;
        out[BMO_SPOT_STAT_N_ROWS] = (double)n;
        out[BMO_SPOT_STAT_CX] = cx;
        out[BMO_SPOT_STAT_CZ] = cz;
        out[BMO_SPOT_STAT_X_MIN] = s.x_min;
        out[BMO_SPOT_STAT_X_MAX] = s.x_max;
        out[BMO_SPOT_STAT_Z_MIN] = s.z_min;
        out[BMO_SPOT_STAT_Z_MAX] = s.z_max;
        cent[c] = make_double2(cx, cz);
    }
};

// second pass of work item blockIdx.x: central moments of its rows about the computed centroid of its configuration
__global__ __launch_bounds__(256) void spot_moments_kernel(const double* __restrict__ rows, int32_t cols, const SplitWork* __restrict__ work,
                                                           const double2* __restrict__ cent, SpotSum2* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const double2 c = cent[W.cfg];
    sum_pass_strided(W, partial, [&](SpotSum2& a, int64_t h) {
        const double* r = rows + h * cols;
        const double dx = r[0] - c.x, dz = r[1] - c.y;
        const double xx = dx * dx, zz = dz * dz;
        a.xx += xx;
        a.zz += zz;
        a.xz += dx * dz;
        const double q = xx + zz;
        a.r2 = q > a.r2 ? q : a.r2;
    });
}

struct SpotMomentsFinish {
    const int64_t* count;
    double* stats;
    __device__ void empty(int32_t) const {}  // NaN already
    __device__ void operator()(int32_t c, const SpotSum2& s) const {
        double* out = stats + (int64_t)c * BMO_SPOT_STAT_N;
        const int64_t n = count[c];
        const double mxx = s.xx / (double)n, mzz = s.zz / (double)n;
        out[BMO_SPOT_STAT_MXX] = mxx;
        out[BMO_SPOT_STAT_MZZ] = mzz;
        out[BMO_SPOT_STAT_MXZ] = s.xz / (double)n;
        out[BMO_SPOT_STAT_RMS_R] = sqrt(mxx + mzz);
        out[BMO_SPOT_STAT_GEO_R] = sqrt(s.r2);
    }
};

}  // namespace

// splits of the n_rows rows of one configuration: at least SPOT_MIN_SPLIT rows each and at most SPOT_MAX_SPLITS of them, every split a
// multiple of 256 rows
// (tests/spot_ref.py restates this function and reads the three constants from this text: keep them in step)
static void spot_splits(int64_t n_rows, int64_t& n_splits, int64_t& rows_per_split) {
    n_splits = (n_rows + SPOT_MIN_SPLIT - 1) / SPOT_MIN_SPLIT;
    if (n_splits > SPOT_MAX_SPLITS) n_splits = SPOT_MAX_SPLITS;
    if (n_splits < 1) n_splits = 1;
    rows_per_split = (n_rows + n_splits - 1) / n_splits;
    rows_per_split = (rows_per_split + 255) / 256 * 256;
    if (rows_per_split < 256) rows_per_split = 256;
    n_splits = n_rows > 0 ? (n_rows + rows_per_split - 1) / rows_per_split : 1;
}

// the plan of a read-out that walks rows without a grid of points (the spot image and every statistics pass): splits by spot_splits
// (which knows no point blocks), no launch batching
static void rows_splits(int64_t n_rows, unsigned, int64_t& n_splits, int64_t& rows_per_split) { spot_splits(n_rows, n_splits, rows_per_split); }
static SplitPlan rows_plan(const Ranges& R) { return SplitPlan(R, 1, rows_splits); }
// the same splits with the launches of a read-out that writes n_pts partial sums per work item
static SplitPlan rows_plan(const Ranges& R, int64_t n_pts) { return SplitPlan(R, 1, n_pts, rows_splits); }

// the work items of such a read-out on the grid's x dimension
static int rows_items(const SplitPlan& plan, const char* who, unsigned& n_items) {
    if (plan.work.size() > (size_t)0x7fffffff) return fail(BMO_ERR_LIMIT, std::string(who) + ": more work items than one launch holds");
    for (int64_t per : plan.per_split)
        if (per > (int64_t)0xffffffff) return fail(BMO_ERR_LIMIT, std::string(who) + ": more rows per split than a 32-bit counter holds");
    n_items = (unsigned)plan.work.size();
    return BMO_OK;
}

// The host side of a read-out that walks its rows in statistics passes, each an accumulate kernel and the reduce of its records: the plan,
// the upload, the stream, the timer and the records.  A read-out makes one, checks items(), adds to `up` what its kernels read besides the
// work list, allocates its own buffers, calls begin(), pass() per pass and end(); everything queues behind one synchronisation.
struct RowPasses {
    SplitPlan plan;
    // What a reduce folds and hands to the Finish: range i is records first_work .. first_work + n_splits - 1.  The configurations' work
    // items, unless the read-out lays its records out otherwise before begin() (the focus statistics: [plane][item]).
    std::vector<SplitCfg> ranges;
    unsigned n_items = 0;
    dim3 grid;  // of an accumulate kernel: the work items on x; y and z are the read-out's to use
    Packed up;
    hipStream_t st = 0;
    EventTimer timer;
    DevBuf records;  // one buffer for every pass: the passes run in stream order, a pass's reduce has read it before the next pass writes
    size_t o_work = 0, o_ranges = 0;

    explicit RowPasses(const Ranges& R) : plan(rows_plan(R)), ranges(plan.cfg) {}
    int items(const char* who) {
        const int rc = rows_items(plan, who, n_items);
        grid = dim3(n_items);
        return rc;
    }
    // uploads, sizes `records` for the largest of the passes' records Recs, starts the timer
    template <class... Recs>
    int begin() {
        o_work = up.add(plan.work), o_ranges = up.add(ranges);
        size_t cells = 0;
        for (const SplitCfg& c : ranges) cells += (size_t)c.n_splits;
        int rc;
        if ((rc = up.upload(st)) || (rc = records.alloc(cells * std::max({sizeof(Recs)...})))) return rc;
        return timer.start(st);
    }
    const SplitWork* work() const { return up.at<SplitWork>(o_work); }
    const SplitCfg* cfg() const { return up.at<SplitCfg>(o_ranges); }
    // kernel(args..., records) on `grid`, when there is a work item at all; the reduce hands the record of every range to `finish`
    template <class Rec, class Kernel, class Finish, class... Args>
    void pass(Kernel kernel, Finish finish, Args... args) {
        if (n_items > 0) hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, args..., (Rec*)records.p);
        sum_reduce<Rec>((unsigned)ranges.size(), st, cfg(), records, finish);
    }
    int end(double* kernel_ms) { return timer.stop(kernel_ms); }
};

// window c as the kernels read it, or why it is refused
static bool spot_window(const double* w, int32_t nx, int32_t nz, SpotWindow& W) {
    for (int q = 0; q < 4; ++q)
        if (!std::isfinite(w[q])) return false;
    if (!(w[1] > w[0] && w[3] > w[2])) return false;
    W = SpotWindow{w[0], w[1], w[2], w[3], (double)nx / (w[1] - w[0]), (double)nz / (w[3] - w[2])};
    return std::isfinite(W.sx) && std::isfinite(W.sz) && W.sx > 0 && W.sz > 0;  // an extent that overflows or underflows has no bin width
}

// The images of the K = R.count.size() configurations from the device rows `rows` [..][cols]: win [K], image [K][nx * nz], outside [K].
static int spot_image_read(const double* rows, int32_t cols, const Ranges& R, const std::vector<SpotWindow>& win, int32_t nx, int32_t nz, int64_t* image,
                           int64_t* outside, double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    const int64_t n_bins = (int64_t)nx * nz;
    hipStream_t st = 0;
    const SplitPlan plan = rows_plan(R);
    unsigned n_items = 0;
    if (int rc = rows_items(plan, who, n_items)) return rc;
    Packed up;
    const size_t o_work = up.add(plan.work), o_win = up.add(win);
    DevBuf d_img, d_out;
    int rc;
    if ((rc = up.upload(st)) || (rc = d_img.alloc(K * (size_t)n_bins * 8)) || (rc = d_out.alloc(K * 8))) return rc;
    EventTimer timer;
    if ((rc = timer.start(st))) return rc;
    HIP_TRY(hipMemsetAsync(d_img.p, 0, K * (size_t)n_bins * 8, st));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, K * 8, st));
    if (n_items > 0) {
        if (n_bins <= SPOT_LDS_BINS)
            hipLaunchKernelGGL(spot_image_kernel<true>, dim3(n_items), dim3(256), (size_t)n_bins * 4, st, rows, cols, up.at<SplitWork>(o_work), up.at<SpotWindow>(o_win), nx,
                               nz, (unsigned long long*)d_img.p, (unsigned long long*)d_out.p);
        else
            hipLaunchKernelGGL(spot_image_kernel<false>, dim3(n_items), dim3(256), 0, st, rows, cols, up.at<SplitWork>(o_work), up.at<SpotWindow>(o_win), nx, nz,
                               (unsigned long long*)d_img.p, (unsigned long long*)d_out.p);
    }
    if ((rc = timer.stop(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(image, d_img.p, K * (size_t)n_bins * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(outside, d_out.p, K * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

// The statistics [K][BMO_SPOT_STAT_N] of the K configurations from the device rows `rows` [..][cols].
static int spot_stats_read(const double* rows, int32_t cols, const Ranges& R, double* stats, double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    RowPasses P(R);
    if (int rc = P.items(who)) return rc;
    const size_t o_count = P.up.add(R.count);
    DevBuf d_stats, d_cent;
    int rc;
    if ((rc = d_stats.alloc(K * BMO_SPOT_STAT_N * 8)) || (rc = d_cent.alloc(K * sizeof(double2))) || (rc = P.begin<SpotSum1, SpotSum2>())) return rc;
    const int64_t* d_count = P.up.at<int64_t>(o_count);
    double* const g_stats = (double*)d_stats.p;
    double2* const g_cent = (double2*)d_cent.p;
    P.pass<SpotSum1>(spot_centroid_kernel, SpotCentroidFinish{d_count, g_stats, g_cent}, rows, cols, P.work());
    P.pass<SpotSum2>(spot_moments_kernel, SpotMomentsFinish{d_count, g_stats}, rows, cols, P.work(), g_cent);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(stats, g_stats, K * BMO_SPOT_STAT_N * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

static bool spot_image_shape_ok(int32_t nx, int32_t nz) { return nx > 0 && nz > 0 && (int64_t)nx * nz <= (int64_t)0x7fffffff; }

extern "C" int bmo_spot_image(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, const double window[4], int32_t nx, int32_t nz,
                              int32_t device, int64_t* image, int64_t* outside, double* kernel_ms) {
    if (!window || !image || !outside || n_rows < 0 || (n_rows > 0 && !rows) || row_cols < 2 || row_cols > 9 || !spot_image_shape_ok(nx, nz))
        return fail(BMO_ERR_INVALID, "bmo_spot_image: bad argument (null pointer, nx or nz <= 0 or nx * nz >= 2^31, row_cols outside 2..9)");
    std::vector<SpotWindow> win(1);
    if (!spot_window(window, nx, nz, win[0])) return fail(BMO_ERR_INVALID, "bmo_spot_image: the window must be finite with x1 > x0 and z1 > z0");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_rows;
    if (int rc = single_rows("bmo_spot_image", rows, n_rows, row_cols, rows_on_device, device, d_rows)) return rc;
    return spot_image_read(rows, row_cols, Ranges{{0}, {n_rows}}, win, nx, nz, image, outside, kernel_ms, "bmo_spot_image");
}

extern "C" int bmo_spot_image_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* windows, int32_t nx, int32_t nz, int64_t* image,
                                    int64_t* outside, double* kernel_ms) {
    if (!res || !windows || !image || !outside || !spot_image_shape_ok(nx, nz))
        return fail(BMO_ERR_INVALID, "bmo_spot_image_sweep: bad argument (null pointer, nx or nz <= 0 or nx * nz >= 2^31)");
    if (int rc = slot_check("bmo_spot_image_sweep", res, detector, BMO_OBJ_SPOTDETECTOR, true, n_configs)) return rc;
    std::vector<SpotWindow> win((size_t)n_configs);
    for (int32_t c = 0; c < n_configs; ++c)
        if (!spot_window(windows + 4 * c, nx, nz, win[(size_t)c]))
            return fail(BMO_ERR_INVALID, "bmo_spot_image_sweep: the window of configuration " + std::to_string(c) + " must be finite with x1 > x0 and z1 > z0");
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_rows = 0
        std::fill(image, image + (size_t)n_configs * (size_t)nx * (size_t)nz, (int64_t)0);
        std::fill(outside, outside + n_configs, (int64_t)0);
        return BMO_OK;
    }
    Ranges R;
    const double* rows;
    if (int rc = resident_rows("bmo_spot_image_sweep", res, detector, H, n_configs, R, rows)) return rc;
    return spot_image_read(rows, 9, R, win, nx, nz, image, outside, kernel_ms, "bmo_spot_image_sweep");
}

extern "C" int bmo_spot_stats(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, int32_t device, double* stats, double* kernel_ms) {
    if (!stats || n_rows < 0 || (n_rows > 0 && !rows) || row_cols < 2 || row_cols > 9)
        return fail(BMO_ERR_INVALID, "bmo_spot_stats: bad argument (null pointer, row_cols outside 2..9)");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_rows;
    if (int rc = single_rows("bmo_spot_stats", rows, n_rows, row_cols, rows_on_device, device, d_rows)) return rc;
    return spot_stats_read(rows, row_cols, Ranges{{0}, {n_rows}}, stats, kernel_ms, "bmo_spot_stats");
}

extern "C" int bmo_spot_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, double* stats, double* kernel_ms) {
    if (!res || !stats) return fail(BMO_ERR_INVALID, "bmo_spot_stats_sweep: bad argument");
    if (int rc = slot_check("bmo_spot_stats_sweep", res, detector, BMO_OBJ_SPOTDETECTOR, true, n_configs)) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_rows = 0
        fill_empty_stats(stats, (size_t)n_configs, BMO_SPOT_STAT_N);
        return BMO_OK;
    }
    Ranges R;
    const double* rows;
    if (int rc = resident_rows("bmo_spot_stats_sweep", res, detector, H, n_configs, R, rows)) return rc;
    return spot_stats_read(rows, 9, R, stats, kernel_ms, "bmo_spot_stats_sweep");
}

// ====================================================================================================================
// Wavefront read-out: the statistics of a PSFDetector's rows (include/bmo.h "Wavefront read-out"): the proj-weighted centroid, the extrema
// and half-widths of calc_local_lims (PSFDetector.jl:115-140), and the wavefront error and Strehl ratio at a reference point of the
// detector plane.  The plumbing of the spot statistics (slot_ranges, rows_plan, work items on the grid's x dimension, sum records: lane /
// shuffle / wave / split order of the sums), three accumulate passes with a per-configuration reduce each, queued behind one synchronisation:
//   A  N, S, sum proj x, sum proj z, the extrema of x, z and k; its reduce leaves the centroid and the reference point p on the device
//   B  half-widths about the computed centroid, sum proj W, F = sum proj cis(k W); writes (proj, W) of every row to a scratch column
//   C  sum proj (W - W_MEAN)^2 and the extrema of W - W_MEAN, from the 16-byte scratch rows instead of the 72-byte rows
// A reduce is sum_reduce_kernel with the pass's Finish: one workgroup per configuration stages the configuration's partial sums through LDS
// and thread 0 folds them in split order (sum_fold).
// Passes A and B use all nine columns and are tile-staged (rows_staged); pass C is strided.
namespace {

#define PSF_STAT_SUM_A(F) \
    F(s, SumAdd) F(sx, SumAdd) F(sz, SumAdd) F(x_min, SumMin) F(x_max, SumMax) F(z_min, SumMin) F(z_max, SumMax) F(k_min, SumMin) F(k_max, SumMax)
#define PSF_STAT_SUM_B(F) F(hwx, SumMax0) F(hwz, SumMax0) F(sw, SumAdd) F(re, SumAdd) F(im, SumAdd)
#define PSF_STAT_SUM_C(F) F(var, SumAdd) F(lo, SumMin) F(hi, SumMax)
SUM_RECORD(PsfStatSumA, PSF_STAT_SUM_A);
SUM_RECORD(PsfStatSumB, PSF_STAT_SUM_B);
SUM_RECORD(PsfStatSumC, PSF_STAT_SUM_C);
// what the later passes need of configuration c
struct PsfStatMid {
    double cx, cz, w_mean;
    d3 p;  // the reference point in world coordinates
};

// local coordinate of row r along axis e (PSFDetector.jl:95-97): dot(hit - origin, e), left to right
__device__ __forceinline__ double psf_local(const double* r, const d3& o, const d3& e) {
    return ((r[0] - o.x) * e.x + (r[1] - o.y) * e.y) + (r[2] - o.z) * e.z;
}

// The terms that the wavefront statistics and the Zernike fit have in common, one definition each, over the sum record of either: run in
// the same lane / wave / split order they make S, X_REF, Z_REF and W_MEAN of the two read-outs equal bit for bit.
// pass A: the proj-weighted centroid sums of row r at local (x, z)
template <class R>
__device__ __forceinline__ void wave_centroid_add(R& a, const double* r, double x, double z) {
    const double w = r[7];
    a.s += w;
    a.sx += w * x;
    a.sz += w * z;
}
// its reduce: the centroid, the reference point (ref_xz: nullptr for the centroid, or [K][2]) and that point in world coordinates
struct WaveRef {
    double cx, cz, x_ref, z_ref;
    d3 p;
};
template <class R>
__device__ __forceinline__ WaveRef wave_ref(const R& a, const PsfPose& P, const double* ref_xz, int32_t c) {
    const double cx = a.sx / a.s, cz = a.sz / a.s;
    const double x_ref = ref_xz ? ref_xz[2 * c] : cx, z_ref = ref_xz ? ref_xz[2 * c + 1] : cz;
    return WaveRef{cx, cz, x_ref, z_ref, psf_point(P.origin, P.e1, P.e2, x_ref, z_ref)};
}
// pass B: W of row r seen from the reference point p, added to sum proj W
template <class R>
__device__ __forceinline__ double wave_path_add(R& b, const d3& p, const double* r) {
    const double path = psf_path(p, r);
    b.sw += r[7] * path;
    return path;
}
// its reduce: W_MEAN over the S of pass A
template <class R>
__device__ __forceinline__ double wave_mean(const R& b, double s) {
    return b.sw / s;
}

// pass A of work item blockIdx.x
__global__ __launch_bounds__(256) void psf_stats_sums_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, const PsfPose* __restrict__ pose,
                                                             PsfStatSumA* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const PsfPose C = pose[W.cfg];
    sum_pass_staged(hits, W, partial, [&](PsfStatSumA& a, const double* r, int64_t) {
        const double x = psf_local(r, C.origin, C.e1), z = psf_local(r, C.origin, C.e2);
        const double k = r[8];
        wave_centroid_add(a, r, x, z);
        a.x_min = x < a.x_min ? x : a.x_min;
        a.x_max = x > a.x_max ? x : a.x_max;
        a.z_min = z < a.z_min ? z : a.z_min;
        a.z_max = z > a.z_max ? z : a.z_max;
        a.k_min = k < a.k_min ? k : a.k_min;
        a.k_max = k > a.k_max ? k : a.k_max;
    });
}

// N, S, the centroid, the extrema and the reference point go to stats[c], what the later passes need to mid[c].  ref_xz: nullptr (the
// centroid) or [K][2]
struct PsfStatSumsFinish {
    const int64_t* count;
    const PsfPose* pose;
    const double* ref_xz;
    double* stats;
    PsfStatMid* mid;
    __device__ void empty(int32_t c) const {
        double* out = stats + (int64_t)c * BMO_PSF_STAT_N;
        out[BMO_PSF_STAT_N_ROWS] = 0.0;
        for (int q = 1; q < BMO_PSF_STAT_N; ++q) out[q] = knan();
        mid[c] = PsfStatMid{0.0, 0.0, 0.0, d3{0.0, 0.0, 0.0}};
    }
    __device__ void operator()(int32_t c, const PsfStatSumA& a) const {
        double* out = stats + (int64_t)c * BMO_PSF_STAT_N;
        out[BMO_PSF_STAT_N_ROWS] = (double)count[c];
        const WaveRef ref = wave_ref(a, pose[c], ref_xz, c);
        out[BMO_PSF_STAT_S] = a.s;
        out[BMO_PSF_STAT_CX] = ref.cx;
        out[BMO_PSF_STAT_CZ] = ref.cz;
        out[BMO_PSF_STAT_X_MIN] = a.x_min;
        out[BMO_PSF_STAT_X_MAX] = a.x_max;
        out[BMO_PSF_STAT_Z_MIN] = a.z_min;
        out[BMO_PSF_STAT_Z_MAX] = a.z_max;
        out[BMO_PSF_STAT_X_REF] = ref.x_ref;
        out[BMO_PSF_STAT_Z_REF] = ref.z_ref;
        out[BMO_PSF_STAT_K_MIN] = a.k_min;
        out[BMO_PSF_STAT_K_MAX] = a.k_max;
        mid[c] = PsfStatMid{ref.cx, ref.cz, 0.0, ref.p};
    }
};

// pass B of work item blockIdx.x; pw[h] = (proj, W) of row h for pass C
__global__ __launch_bounds__(256) void psf_stats_wave_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, const PsfPose* __restrict__ pose,
                                                             const PsfStatMid* __restrict__ mid, double2* __restrict__ pw, PsfStatSumB* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const PsfPose C = pose[W.cfg];
    const PsfStatMid M = mid[W.cfg];
    sum_pass_staged(hits, W, partial, [&](PsfStatSumB& b, const double* r, int64_t h) {
        const double ax = fabs(psf_local(r, C.origin, C.e1) - M.cx), az = fabs(psf_local(r, C.origin, C.e2) - M.cz);
        b.hwx = ax > b.hwx ? ax : b.hwx;
        b.hwz = az > b.hwz ? az : b.hwz;
        const double w = r[7];
        const double path = wave_path_add(b, M.p, r);
        const double phase = r[8] * path;
        double sn, cs;
        sincos(phase, &sn, &cs);
        b.re += w * cs;
        b.im += w * sn;
        pw[h] = make_double2(w, path);
    });
}

struct PsfStatWaveFinish {
    double* stats;
    PsfStatMid* mid;
    __device__ void empty(int32_t) const {}  // NaN already
    __device__ void operator()(int32_t c, const PsfStatSumB& b) const {
        double* out = stats + (int64_t)c * BMO_PSF_STAT_N;
        const double s = out[BMO_PSF_STAT_S];
        const double w_mean = wave_mean(b, s);
        out[BMO_PSF_STAT_HWX] = b.hwx;
        out[BMO_PSF_STAT_HWZ] = b.hwz;
        out[BMO_PSF_STAT_W_MEAN] = w_mean;
        out[BMO_PSF_STAT_F_RE] = b.re;
        out[BMO_PSF_STAT_F_IM] = b.im;
        out[BMO_PSF_STAT_STREHL] = (b.re * b.re + b.im * b.im) / (s * s);
        mid[c].w_mean = w_mean;
    }
};

// pass C of work item blockIdx.x, on the scratch column of pass B
__global__ __launch_bounds__(256) void psf_stats_spread_kernel(const double2* __restrict__ pw, const SplitWork* __restrict__ work, const PsfStatMid* __restrict__ mid,
                                                               PsfStatSumC* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const double w_mean = mid[W.cfg].w_mean;
    sum_pass_strided(W, partial, [&](PsfStatSumC& s, int64_t h) {
        const double2 v = pw[h];
        const double d = v.y - w_mean;
        s.var += v.x * (d * d);
        s.lo = d < s.lo ? d : s.lo;
        s.hi = d > s.hi ? d : s.hi;
    });
}

struct PsfStatSpreadFinish {
    double* stats;
    __device__ void empty(int32_t) const {}  // NaN already
    __device__ void operator()(int32_t c, const PsfStatSumC& s) const {
        double* out = stats + (int64_t)c * BMO_PSF_STAT_N;
        out[BMO_PSF_STAT_W_RMS] = sqrt(s.var / out[BMO_PSF_STAT_S]);
        out[BMO_PSF_STAT_W_LO] = s.lo;
        out[BMO_PSF_STAT_W_HI] = s.hi;
    }
};

}  // namespace

// The statistics [K][BMO_PSF_STAT_N] of the K configurations from the n_rows device rows `hits` [..][9]: poses [K][3], ref_xz nullptr or [K][2].
static int psf_stats_read(const double* hits, int64_t n_rows, const Ranges& R, const double* origins, const double* e1s, const double* e2s, const double* ref_xz,
                          double* stats, double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    RowPasses P(R);
    if (int rc = P.items(who)) return rc;
    const size_t o_count = P.up.add(R.count), o_pose = P.up.add(psf_poses(K, origins, e1s, e2s)), o_ref = ref_xz ? P.up.add(ref_xz, 2 * K) : 0;
    DevBuf d_stats, d_mid, d_pw;
    int rc;
    if ((rc = d_stats.alloc(K * BMO_PSF_STAT_N * 8)) || (rc = d_mid.alloc(K * sizeof(PsfStatMid))) || (rc = d_pw.alloc((size_t)n_rows * sizeof(double2))) ||
        (rc = P.begin<PsfStatSumA, PsfStatSumB, PsfStatSumC>()))
        return rc;
    const PsfPose* d_pose = P.up.at<PsfPose>(o_pose);
    double* const g_stats = (double*)d_stats.p;
    PsfStatMid* const g_mid = (PsfStatMid*)d_mid.p;
    double2* const g_pw = (double2*)d_pw.p;
    P.pass<PsfStatSumA>(psf_stats_sums_kernel,
                        PsfStatSumsFinish{P.up.at<int64_t>(o_count), d_pose, ref_xz ? P.up.at<double>(o_ref) : (const double*)nullptr, g_stats, g_mid}, hits, P.work(),
                        d_pose);
    P.pass<PsfStatSumB>(psf_stats_wave_kernel, PsfStatWaveFinish{g_stats, g_mid}, hits, P.work(), d_pose, g_mid, g_pw);
    P.pass<PsfStatSumC>(psf_stats_spread_kernel, PsfStatSpreadFinish{g_stats}, g_pw, P.work(), g_mid);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(stats, g_stats, K * BMO_PSF_STAT_N * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_stats(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                             const double* ref_xz, int32_t device, double* stats, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !stats || n_hits < 0 || (n_hits > 0 && !hits)) return fail(BMO_ERR_INVALID, "bmo_psf_stats: bad argument (null pointer, n_hits < 0)");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_stats", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    return psf_stats_read(hits, n_hits, Ranges{{0}, {n_hits}}, origin, e1, e2, ref_xz, stats, kernel_ms, "bmo_psf_stats");
}

extern "C" int bmo_psf_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                   const double* ref_xz, double* stats, double* kernel_ms) {
    if (!res || !origins || !e1s || !e2s || !stats) return fail(BMO_ERR_INVALID, "bmo_psf_stats_sweep: bad argument");
    if (int rc = slot_check("bmo_psf_stats_sweep", res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_hits = 0
        fill_empty_stats(stats, (size_t)n_configs, BMO_PSF_STAT_N);
        return BMO_OK;
    }
    Ranges R;
    const double* hits;
    if (int rc = resident_rows("bmo_psf_stats_sweep", res, detector, H, n_configs, R, hits)) return rc;
    return psf_stats_read(hits, H, R, origins, e1s, e2s, ref_xz, stats, kernel_ms, "bmo_psf_stats_sweep");
}

// ====================================================================================================================
// Zernike read-out: the least-squares Zernike coefficients of a PSFDetector's wavefront (include/bmo.h "Zernike read-out").  The plumbing
// and the first two passes are those of the wavefront statistics: both read-outs call wave_centroid_add, wave_ref, wave_path_add and
// wave_mean in the same lane / wave / split order, so S, X_REF, Z_REF and W_MEAN are that call's bit for bit by construction.  Four accumulate
// passes with a per-configuration reduce each, queued behind one synchronisation:
//   A  S, sum proj x, sum proj z, sum proj u, sum proj v over the 9-column rows; its reduce leaves p, U0, V0
//   B  sum proj W and the largest squared pupil radius; writes (proj, W, u, v) of every row to a 32-byte scratch column; its reduce
//      leaves W_MEAN and RHO
//   C  the Gram matrix of the augmented columns (Z_0 .. Z_{J-1}, D): per tile of 256 rows every lane evaluates the columns of its own row
//      into LDS, then every thread owns a 2 x 2 block of the (J + 1)(J + 2) / 2 entries and walks the tile's rows in row order, its accumulators
//      carried across the tiles of the work item: an entry of a work item is the left fold over its rows.  Its reduce folds the work items
//      in split order, one thread per entry, and thread 0 runs the Cholesky solve from LDS.  No float atomics.
//   D  the residual sums and extrema and N_OUT from the scratch column and the coefficients
// The order is a template parameter of the kernels that evaluate terms: every loop over terms unrolls, the terms live in registers.
namespace {

constexpr int ZERN_MAX_J = (BMO_ZERNIKE_MAX_ORDER + 1) * (BMO_ZERNIKE_MAX_ORDER + 2) / 2;  // 28
constexpr int ZERN_MAX_E = (ZERN_MAX_J + 1) * (ZERN_MAX_J + 2) / 2;                        // 435
constexpr int ZERN_ROW_BATCH = 8;    // tile rows whose LDS reads are in flight together in pass C
constexpr int ZERN_FOLD_BATCH = 16;  // partial sums of one entry in flight in pass C's reduce
constexpr int zern_terms_of(int order) { return (order + 1) * (order + 2) / 2; }
// doubles per row of pass C's tile: the J + 1 augmented columns and proj, padded to an odd count (the lanes' writes of one column then
// spread over the banks; the reads of a wave go to one row, whose columns are distinct banks as it is shorter than the 64 banks)
constexpr int zern_row_stride(int order) { return (zern_terms_of(order) + 2) | 1; }

constexpr double zern_fact(int k) {
    double f = 1.0;
    for (int q = 2; q <= k; ++q) f *= q;
    return f;
}
// q_s of R_n^am(rho) / rho^am as a polynomial in t = rho^2 (integers, exact in FP64)
constexpr double zern_q(int n, int am, int s) {
    const int K = (n - am) / 2;
    return (((K - s) & 1) ? -1.0 : 1.0) * (zern_fact(n - K + s) / (zern_fact(K - s) * zern_fact((n + am) / 2 - K + s) * zern_fact(s)));
}
// sqrt((double)k), correctly rounded, k = 0 .. 14
constexpr double ZERN_SQRT[15] = {0.0,
                                  1.0,
                                  1.4142135623730951,
                                  1.7320508075688772,
                                  2.0,
                                  2.23606797749979,
                                  2.449489742783178,
                                  2.6457513110645907,
                                  2.8284271247461903,
                                  3.0,
                                  3.1622776601683795,
                                  3.3166247903554,
                                  3.4641016151377544,
                                  3.605551275463989,
                                  3.7416573867739413};
constexpr double zern_norm(int n, int m) { return ZERN_SQRT[m == 0 ? n + 1 : 2 * (n + 1)]; }

// Horner steps s = S .. 0 of the radial polynomial: r = r * t + q_s.  q_s is a constant expression, so it is a literal in the code.
template <int N, int AM, int S>
__device__ __forceinline__ double zern_horner(double r, double t) {
    if constexpr (S < 0) {
        return r;
    } else {
        constexpr double q = zern_q(N, AM, S);
        return zern_horner<N, AM, S - 1>(r * t + q, t);
    }
}
// One term: Z = N * (r * A) with Horner in t from the top.
template <int N, int M>
__device__ __forceinline__ double zern_term(double t, const double* Cc, const double* Sc) {
    constexpr int AM = M < 0 ? -M : M, K = (N - AM) / 2;
    constexpr double q_top = zern_q(N, AM, K), nrm = zern_norm(N, M);
    const double r = zern_horner<N, AM, K - 1>(q_top, t);
    return nrm * (r * (M >= 0 ? Cc[AM] : Sc[AM]));
}
template <int N, int M, int ORDER, class F>
__device__ __forceinline__ void zern_walk(double t, const double* Cc, const double* Sc, F&& f) {
    if constexpr (N <= ORDER) {
        f((N * (N + 2) + M) / 2, zern_term<N, M>(t, Cc, Sc));
        if constexpr (M + 2 <= N) zern_walk<N, M + 2, ORDER>(t, Cc, Sc, f);
        else zern_walk<N + 1, -(N + 1), ORDER>(t, Cc, Sc, f);
    }
}
// f(j, Z_j(x, y)) for j = 0 .. J - 1 in ascending j; j is a constant in every call
template <int ORDER, class F>
__device__ __forceinline__ void zern_terms(double x, double y, F&& f) {
    const double t = x * x + y * y;
    double Cc[ORDER + 1], Sc[ORDER + 1];
    Cc[0] = 1.0;
    Sc[0] = 0.0;
#pragma unroll
    for (int k = 0; k < ORDER; ++k) {
        Cc[k + 1] = Cc[k] * x - Sc[k] * y;
        Sc[k + 1] = Sc[k] * x + Cc[k] * y;
    }
    zern_walk<0, 0, ORDER>(t, Cc, Sc, f);
}

#define ZERN_SUM_A(F) F(s, SumAdd) F(sx, SumAdd) F(sz, SumAdd) F(su, SumAdd) F(sv, SumAdd)
#define ZERN_SUM_B(F) F(sw, SumAdd) F(r2, SumMax0)
#define ZERN_SUM_D(F) F(var, SumAdd) F(lo, SumMin) F(hi, SumMax) F(n_out, SumAdd)
SUM_RECORD(ZernSumA, ZERN_SUM_A);
SUM_RECORD(ZernSumB, ZERN_SUM_B);
SUM_RECORD(ZernSumD, ZERN_SUM_D);
// what the later passes need of configuration c
struct ZernMid {
    d3 p;  // the reference point in world coordinates
    double u0, v0, rho, w_mean;
};

// direction cosine of row r along axis e
__device__ __forceinline__ double zern_cosine(const double* r, const d3& e) { return (r[3] * e.x + r[4] * e.y) + r[5] * e.z; }

// pass A of work item blockIdx.x
__global__ __launch_bounds__(256) void psf_zernike_sums_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, const PsfPose* __restrict__ pose,
                                                               ZernSumA* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const PsfPose C = pose[W.cfg];
    sum_pass_staged(hits, W, partial, [&](ZernSumA& a, const double* r, int64_t) {
        wave_centroid_add(a, r, psf_local(r, C.origin, C.e1), psf_local(r, C.origin, C.e2));
        a.su += r[7] * zern_cosine(r, C.e1);
        a.sv += r[7] * zern_cosine(r, C.e2);
    });
}

// ref_xz: nullptr (the centroid) or [K][2]; pupil: nullptr or [K][3].  A configuration without rows gets its whole answer here: N = 0,
// STATUS = 1, NaN elsewhere.
struct ZernSumsFinish {
    const int64_t* count;
    const PsfPose* pose;
    const double *ref_xz, *pupil;
    double* info;
    ZernMid* mid;
    __device__ void empty(int32_t c) const {
        double* out = info + (int64_t)c * BMO_ZERNIKE_INFO_N;
        for (int q = 0; q < BMO_ZERNIKE_INFO_N; ++q) out[q] = knan();
        out[BMO_ZERNIKE_N_ROWS] = 0.0;
        out[BMO_ZERNIKE_STATUS] = 1.0;
        mid[c] = ZernMid{d3{0.0, 0.0, 0.0}, 0.0, 0.0, 0.0, 0.0};
    }
    __device__ void operator()(int32_t c, const ZernSumA& a) const {
        double* out = info + (int64_t)c * BMO_ZERNIKE_INFO_N;
        const WaveRef ref = wave_ref(a, pose[c], ref_xz, c);
        const double u0 = pupil ? pupil[3 * c] : a.su / a.s, v0 = pupil ? pupil[3 * c + 1] : a.sv / a.s;
        out[BMO_ZERNIKE_N_ROWS] = (double)count[c];
        out[BMO_ZERNIKE_STATUS] = 0.0;
        out[BMO_ZERNIKE_S] = a.s;
        out[BMO_ZERNIKE_X_REF] = ref.x_ref;
        out[BMO_ZERNIKE_Z_REF] = ref.z_ref;
        out[BMO_ZERNIKE_U0] = u0;
        out[BMO_ZERNIKE_V0] = v0;
        mid[c] = ZernMid{ref.p, u0, v0, 0.0, 0.0};
    }
};

// pass B of work item blockIdx.x; col[h] = (proj, W, u, v) of row h for passes C and D
__global__ __launch_bounds__(256) void psf_zernike_wave_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, const PsfPose* __restrict__ pose,
                                                               const ZernMid* __restrict__ mid, double4* __restrict__ col, ZernSumB* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const PsfPose C = pose[W.cfg];
    const ZernMid M = mid[W.cfg];
    sum_pass_staged(hits, W, partial, [&](ZernSumB& b, const double* r, int64_t h) {
        const double path = wave_path_add(b, M.p, r);
        const double u = zern_cosine(r, C.e1), v = zern_cosine(r, C.e2);
        const double q = (u - M.u0) * (u - M.u0) + (v - M.v0) * (v - M.v0);
        b.r2 = q > b.r2 ? q : b.r2;
        col[h] = make_double4(r[7], path, u, v);
    });
}

struct ZernWaveFinish {
    const double* pupil;
    double* info;
    ZernMid* mid;
    __device__ void empty(int32_t) const {}  // answered already
    __device__ void operator()(int32_t c, const ZernSumB& b) const {
        double* out = info + (int64_t)c * BMO_ZERNIKE_INFO_N;
        const double w_mean = wave_mean(b, out[BMO_ZERNIKE_S]);
        const double rho = pupil ? pupil[3 * c + 2] : sqrt(b.r2);
        out[BMO_ZERNIKE_W_MEAN] = w_mean;
        out[BMO_ZERNIKE_RHO] = rho;
        mid[c].w_mean = w_mean;
        mid[c].rho = rho;
    }
};

// entry e of the packed lower triangle: (i, k), i >= k
__device__ __forceinline__ void zern_entry(int e, int& i, int& k) {
    i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    k = e - i * (i + 1) / 2;
}

// pass C of work item blockIdx.x: partial[blockIdx.x][e] = the left fold of (proj * B_i) * B_k over its rows.  A thread owns a 2 x 2 block of
// entries, columns (2 bi, 2 bi + 1) x (2 bk, 2 bk + 1) with bi >= bk: five LDS reads per row (proj and four columns) feed its four products,
// and every entry is still the sum over the rows in row order.  The reads are volatile so that each stays a single-address 8-byte read
// (64 banks; the columns of one tile row are distinct banks): left to itself the compiler pairs the reads of unrolled rows into
// two-address reads, which see 32 banks and conflict.
template <int ORDER>
__global__ __launch_bounds__(256) void psf_zernike_gram_kernel(const double4* __restrict__ col, const SplitWork* __restrict__ work, const ZernMid* __restrict__ mid,
                                                               double* __restrict__ partial) {
    constexpr int J = zern_terms_of(ORDER), NC = J + 1, E = (J + 1) * (J + 2) / 2, STRIDE = zern_row_stride(ORDER);
    constexpr int NB = (NC + 1) / 2, NBLK = NB * (NB + 1) / 2;  // at most 15 block rows, 120 blocks
    __shared__ double tile[PSF_TILE * STRIDE];
    const SplitWork W = work[blockIdx.x];
    const ZernMid M = mid[W.cfg];
    const bool owner = (int)threadIdx.x < NBLK;
    int bi, bk;
    zern_entry(owner ? (int)threadIdx.x : 0, bi, bk);
    const int i0 = 2 * bi, k0 = 2 * bk;
    const bool has_i1 = i0 + 1 < NC, has_k1 = k0 + 1 < NC;
    const int i1 = has_i1 ? i0 + 1 : i0, k1 = has_k1 ? k0 + 1 : k0;  // a column past the last one reads its neighbour and is not written
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    for (int64_t base = W.h0; base < W.h1; base += PSF_TILE) {
        const int cnt = (int)(W.h1 - base < PSF_TILE ? W.h1 - base : PSF_TILE);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const double4 q = col[base + threadIdx.x];
            double* row = tile + STRIDE * threadIdx.x;
            const double x = (q.z - M.u0) / M.rho, y = (q.w - M.v0) / M.rho;
            zern_terms<ORDER>(x, y, [&](int j, double Z) { row[j] = Z; });
            row[J] = q.y - M.w_mean;
            row[J + 1] = q.x;
        }
        __syncthreads();
        if (owner) {
            auto add_row = [&](double p, double bi0, double bi1, double bk0, double bk1) {
                const double pi0 = p * bi0, pi1 = p * bi1;
                a00 += pi0 * bk0;
                a01 += pi0 * bk1;
                a10 += pi1 * bk0;
                a11 += pi1 * bk1;
            };
            // the reads of ZERN_ROW_BATCH rows are issued together, then the rows are added in row order: one LDS latency per batch
            int h = 0;
            for (; h + ZERN_ROW_BATCH <= cnt; h += ZERN_ROW_BATCH) {
                double p[ZERN_ROW_BATCH], bi0[ZERN_ROW_BATCH], bi1[ZERN_ROW_BATCH], bk0[ZERN_ROW_BATCH], bk1[ZERN_ROW_BATCH];
#pragma unroll
                for (int q = 0; q < ZERN_ROW_BATCH; ++q) {
                    const volatile double* row = tile + STRIDE * (h + q);
                    p[q] = row[J + 1], bi0[q] = row[i0], bi1[q] = row[i1], bk0[q] = row[k0], bk1[q] = row[k1];
                }
#pragma unroll
                for (int q = 0; q < ZERN_ROW_BATCH; ++q) add_row(p[q], bi0[q], bi1[q], bk0[q], bk1[q]);
            }
            for (; h < cnt; ++h) {
                const volatile double* row = tile + STRIDE * h;
                const double p = row[J + 1], bi0 = row[i0], bi1 = row[i1], bk0 = row[k0], bk1 = row[k1];
                add_row(p, bi0, bi1, bk0, bk1);
            }
        }
    }
    if (!owner) return;
    double* out = partial + (int64_t)blockIdx.x * E;
    out[i0 * (i0 + 1) / 2 + k0] = a00;
    if (has_k1 && k0 + 1 <= i0) out[i0 * (i0 + 1) / 2 + k0 + 1] = a01;  // above the diagonal in a diagonal block
    if (has_i1) {
        out[(i0 + 1) * (i0 + 2) / 2 + k0] = a10;
        if (has_k1) out[(i0 + 1) * (i0 + 2) / 2 + k0 + 1] = a11;
    }
}

// configuration blockIdx.x: the work items' Gram entries folded in split order, one thread per entry; thread 0 then solves (the loops of
// include/bmo.h) from LDS and writes coef, STATUS and gram.  J terms; gram: nullptr or [K][E].
__global__ __launch_bounds__(256) void psf_zernike_gram_reduce_kernel(const SplitCfg* __restrict__ cfg, const int64_t* __restrict__ count, int32_t J,
                                                                      const double* __restrict__ partial, double* __restrict__ info, double* __restrict__ coef,
                                                                      double* __restrict__ gram) {
    __shared__ double G[ZERN_MAX_E];
    __shared__ double L[ZERN_MAX_J * (ZERN_MAX_J + 1) / 2];
    __shared__ double yv[ZERN_MAX_J];
    const int32_t c = (int32_t)blockIdx.x;
    const int E = (J + 1) * (J + 2) / 2;
    const int64_t n = count[c];
    double* cf = coef + (int64_t)c * J;
    if (n == 0) {
        for (int q = threadIdx.x; q < J; q += 256) cf[q] = knan();
        if (gram)
            for (int q = threadIdx.x; q < E; q += 256) gram[(int64_t)c * E + q] = knan();
        return;
    }
    const SplitCfg C = cfg[c];
    // an entry's partial sums lie E doubles apart; ZERN_FOLD_BATCH loads are issued together and then added in split order, so the thread
    // waits for memory once per batch and not once per work item
    for (int e = threadIdx.x; e < E; e += 256) {
        const double* src = partial + C.first_work * E + e;
        double g = 0.0;
        int s = 0;
        for (; s + ZERN_FOLD_BATCH <= C.n_splits; s += ZERN_FOLD_BATCH) {
            double v[ZERN_FOLD_BATCH];
#pragma unroll
            for (int q = 0; q < ZERN_FOLD_BATCH; ++q) v[q] = src[(int64_t)(s + q) * E];
#pragma unroll
            for (int q = 0; q < ZERN_FOLD_BATCH; ++q) g += v[q];
        }
        for (; s < C.n_splits; ++s) g += src[(int64_t)s * E];
        G[e] = g;
        if (gram) gram[(int64_t)c * E + e] = g;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* out = info + (int64_t)c * BMO_ZERNIKE_INFO_N;
    const double rho = out[BMO_ZERNIKE_RHO];
    int status = 0;
    if (n < J || rho == 0.0 || !isfinite(rho)) status = 1;
    for (int j = 0; j < J && status == 0; ++j) {
        const double* Lj = L + j * (j + 1) / 2;
        double d = G[j * (j + 1) / 2 + j];
        for (int k = 0; k < j; ++k) d = d - Lj[k] * Lj[k];
        if (!(d > 0.0)) {
            status = 2;
            break;
        }
        const double ljj = sqrt(d);
        L[j * (j + 1) / 2 + j] = ljj;
        for (int i = j + 1; i < J; ++i) {
            double* Li = L + i * (i + 1) / 2;
            double s = G[i * (i + 1) / 2 + j];
            for (int k = 0; k < j; ++k) s = s - Li[k] * Lj[k];
            Li[j] = s / ljj;
        }
    }
    out[BMO_ZERNIKE_STATUS] = (double)status;
    if (status != 0) {
        for (int q = 0; q < J; ++q) cf[q] = knan();
        return;
    }
    const double* b = G + J * (J + 1) / 2;
    for (int i = 0; i < J; ++i) {
        const double* Li = L + i * (i + 1) / 2;
        double s = b[i];
        for (int k = 0; k < i; ++k) s = s - Li[k] * yv[k];
        yv[i] = s / Li[i];
    }
    for (int i = J - 1; i >= 0; --i) {  // c overwrites y from the top
        double s = yv[i];
        for (int k = i + 1; k < J; ++k) s = s - L[k * (k + 1) / 2 + i] * yv[k];
        yv[i] = s / L[i * (i + 1) / 2 + i];
    }
    for (int q = 0; q < J; ++q) cf[q] = yv[q];
}

// The residual of one row of the scratch column about the surface cf [J], one definition for the Zernike read-out's pass D and the OPD map's
// passes E and M: the pupil coordinates (x, y) of the row and E_h = (W_h - W_MEAN) - F_h.
template <int ORDER>
__device__ __forceinline__ double zern_residual(const double4& q, const ZernMid& M, const double* cf, double& x, double& y) {
    x = (q.z - M.u0) / M.rho, y = (q.w - M.v0) / M.rho;
    double f = 0.0;
    zern_terms<ORDER>(x, y, [&](int j, double Z) { f = j == 0 ? cf[0] * Z : f + cf[j] * Z; });
    return (q.y - M.w_mean) - f;
}
// the residual sums of that row added to a record with the fields of ZERN_SUM_D; returns E_h
template <int ORDER, class R>
__device__ __forceinline__ double zern_residual_add(R& s, const double4& q, const ZernMid& M, const double* cf) {
    double x, y;
    const double e = zern_residual<ORDER>(q, M, cf, x, y);
    const double t = x * x + y * y;
    s.var += q.x * (e * e);
    s.lo = e < s.lo ? e : s.lo;
    s.hi = e > s.hi ? e : s.hi;
    s.n_out += t > 1.0 ? 1.0 : 0.0;
    return e;
}

// pass D of work item blockIdx.x, on the scratch column: the residual of the fit
template <int ORDER>
__global__ __launch_bounds__(256) void psf_zernike_residual_kernel(const double4* __restrict__ col, const SplitWork* __restrict__ work, const ZernMid* __restrict__ mid,
                                                                   const double* __restrict__ coef, ZernSumD* __restrict__ partial) {
    constexpr int J = zern_terms_of(ORDER);
    const SplitWork W = work[blockIdx.x];
    const ZernMid M = mid[W.cfg];
    double cf[J];
#pragma unroll
    for (int j = 0; j < J; ++j) cf[j] = coef[(int64_t)W.cfg * J + j];
    sum_pass_strided(W, partial, [&](ZernSumD& s, int64_t h) { zern_residual_add<ORDER>(s, col[h], M, cf); });
}

struct ZernResidualFinish {
    double* info;
    __device__ void empty(int32_t) const {}  // answered already
    __device__ void operator()(int32_t c, const ZernSumD& s) const {
        double* out = info + (int64_t)c * BMO_ZERNIKE_INFO_N;
        const bool solved = out[BMO_ZERNIKE_STATUS] == 0.0;
        out[BMO_ZERNIKE_FIT_RMS] = solved ? sqrt(s.var / out[BMO_ZERNIKE_S]) : knan();
        out[BMO_ZERNIKE_E_LO] = solved ? s.lo : knan();
        out[BMO_ZERNIKE_E_HI] = solved ? s.hi : knan();
        out[BMO_ZERNIKE_N_OUT] = s.n_out;
    }
};

}  // namespace

// what a configuration without rows reads: N = 0, STATUS = 1, NaN elsewhere
static void psf_zernike_empty(int32_t n_configs, int32_t J, double* coef, double* info, double* gram) {
    const size_t E = (size_t)(J + 1) * (J + 2) / 2;
    std::fill(coef, coef + (size_t)n_configs * J, std::nan(""));
    if (gram) std::fill(gram, gram + (size_t)n_configs * E, std::nan(""));
    fill_empty_stats(info, (size_t)n_configs, BMO_ZERNIKE_INFO_N);
    for (int32_t c = 0; c < n_configs; ++c) info[(size_t)c * BMO_ZERNIKE_INFO_N + BMO_ZERNIKE_STATUS] = 1.0;
}

// order in range and every given pupil (U0, V0, RHO) usable
static bool psf_zernike_args_ok(const double* pupil, int32_t n_configs, int32_t order) {
    if (order < 0 || order > BMO_ZERNIKE_MAX_ORDER) return false;
    for (int32_t c = 0; pupil && c < n_configs; ++c) {
        const double* q = pupil + 3 * c;
        if (!std::isfinite(q[0]) || !std::isfinite(q[1]) || !std::isfinite(q[2]) || !(q[2] > 0)) return false;
    }
    return true;
}

// The fits of the K configurations from the n_rows device rows `hits` [..][9]: poses [K][3], ref_xz nullptr or [K][2], pupil nullptr or [K][3];
// coef [K][J], info [K][BMO_ZERNIKE_INFO_N], gram nullptr or [K][(J + 1)(J + 2) / 2].
static int psf_zernike_read(const double* hits, int64_t n_rows, const Ranges& R, const double* origins, const double* e1s, const double* e2s, const double* ref_xz,
                            const double* pupil, int32_t order, double* coef, double* info, double* gram, double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    const int32_t J = zern_terms_of(order);
    const size_t E = (size_t)(J + 1) * (J + 2) / 2;
    RowPasses P(R);
    if (int rc = P.items(who)) return rc;
    const size_t o_count = P.up.add(R.count), o_pose = P.up.add(psf_poses(K, origins, e1s, e2s));
    const size_t o_ref = ref_xz ? P.up.add(ref_xz, 2 * K) : 0, o_pupil = pupil ? P.up.add(pupil, 3 * K) : 0;
    DevBuf d_gram_parts, d_info, d_coef, d_gram, d_mid, d_col;
    int rc;
    if ((rc = d_gram_parts.alloc((size_t)P.n_items * E * 8)) || (rc = d_info.alloc(K * BMO_ZERNIKE_INFO_N * 8)) || (rc = d_coef.alloc(K * (size_t)J * 8)) ||
        (gram && (rc = d_gram.alloc(K * E * 8))) || (rc = d_mid.alloc(K * sizeof(ZernMid))) || (rc = d_col.alloc((size_t)n_rows * sizeof(double4))) ||
        (rc = P.begin<ZernSumA, ZernSumB, ZernSumD>()))
        return rc;
    const int64_t* d_count = P.up.at<int64_t>(o_count);
    const PsfPose* d_pose = P.up.at<PsfPose>(o_pose);
    const double* d_pupil = pupil ? P.up.at<double>(o_pupil) : (const double*)nullptr;
    double* const g_info = (double*)d_info.p;
    ZernMid* const g_mid = (ZernMid*)d_mid.p;
    double4* const g_col = (double4*)d_col.p;
    P.pass<ZernSumA>(psf_zernike_sums_kernel, ZernSumsFinish{d_count, d_pose, ref_xz ? P.up.at<double>(o_ref) : (const double*)nullptr, d_pupil, g_info, g_mid}, hits,
                     P.work(), d_pose);
    P.pass<ZernSumB>(psf_zernike_wave_kernel, ZernWaveFinish{d_pupil, g_info, g_mid}, hits, P.work(), d_pose, g_mid, g_col);
    // pass C keeps no sum record: the Gram entries have a kernel and a reduce of their own
    void (*const gram_pass[])(const double4*, const SplitWork*, const ZernMid*, double*) = {
        psf_zernike_gram_kernel<0>, psf_zernike_gram_kernel<1>, psf_zernike_gram_kernel<2>, psf_zernike_gram_kernel<3>,
        psf_zernike_gram_kernel<4>, psf_zernike_gram_kernel<5>, psf_zernike_gram_kernel<6>};
    if (P.n_items > 0) hipLaunchKernelGGL(gram_pass[order], P.grid, dim3(256), 0, P.st, g_col, P.work(), g_mid, (double*)d_gram_parts.p);
    hipLaunchKernelGGL(psf_zernike_gram_reduce_kernel, dim3((unsigned)K), dim3(256), 0, P.st, P.cfg(), d_count, J, (const double*)d_gram_parts.p, g_info,
                       (double*)d_coef.p, gram ? (double*)d_gram.p : (double*)nullptr);
    void (*const residual[])(const double4*, const SplitWork*, const ZernMid*, const double*, ZernSumD*) = {
        psf_zernike_residual_kernel<0>, psf_zernike_residual_kernel<1>, psf_zernike_residual_kernel<2>, psf_zernike_residual_kernel<3>,
        psf_zernike_residual_kernel<4>, psf_zernike_residual_kernel<5>, psf_zernike_residual_kernel<6>};
    P.pass<ZernSumD>(residual[order], ZernResidualFinish{g_info}, g_col, P.work(), g_mid, (const double*)d_coef.p);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(info, d_info.p, K * BMO_ZERNIKE_INFO_N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(coef, d_coef.p, K * (size_t)J * 8, hipMemcpyDeviceToHost));
    if (gram) HIP_TRY(hipMemcpy(gram, d_gram.p, K * E * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_zernike(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                               const double* ref_xz, const double* pupil, int32_t order, int32_t device, double* coef, double* info, double* gram,
                               double* kernel_ms) {
    if (!origin || !e1 || !e2 || !coef || !info || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_zernike: bad argument (null pointer, n_hits < 0)");
    if (!psf_zernike_args_ok(pupil, 1, order))
        return fail(BMO_ERR_INVALID, "bmo_psf_zernike: order must be 0 .. 6, a given pupil (U0, V0, RHO) finite with RHO > 0");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_zernike", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    return psf_zernike_read(hits, n_hits, Ranges{{0}, {n_hits}}, origin, e1, e2, ref_xz, pupil, order, coef, info, gram, kernel_ms, "bmo_psf_zernike");
}

extern "C" int bmo_psf_zernike_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                     const double* ref_xz, const double* pupil, int32_t order, double* coef, double* info, double* gram, double* kernel_ms) {
    if (!res || !origins || !e1s || !e2s || !coef || !info) return fail(BMO_ERR_INVALID, "bmo_psf_zernike_sweep: bad argument");
    if (int rc = slot_check("bmo_psf_zernike_sweep", res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    if (!psf_zernike_args_ok(pupil, n_configs, order))
        return fail(BMO_ERR_INVALID, "bmo_psf_zernike_sweep: order must be 0 .. 6, every given pupil (U0, V0, RHO) finite with RHO > 0");
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_hits = 0
        psf_zernike_empty(n_configs, zern_terms_of(order), coef, info, gram);
        return BMO_OK;
    }
    Ranges R;
    const double* hits;
    if (int rc = resident_rows("bmo_psf_zernike_sweep", res, detector, H, n_configs, R, hits)) return rc;
    return psf_zernike_read(hits, H, R, origins, e1s, e2s, ref_xz, pupil, order, coef, info, gram, kernel_ms, "bmo_psf_zernike_sweep");
}

// ====================================================================================================================
// OPD map read-out: the wavefront of a PSFDetector's rows less a given Zernike surface, binned over the pupil square (include/bmo.h "OPD map
// read-out").  Passes A and B are the Zernike read-out's kernels and finish functors, unchanged, writing a Zernike info row that stays on
// the device; then
//   E  psf_zernike_residual_kernel's row body (zern_residual_add) with MQ, MP and N_BAD added to the record; its reduce writes the info
//      columns up to N_BAD and leaves the two scales and STATUS on the device
//   M  the binning: one workgroup per work item, every lane evaluates E_h of its row again, its bin and the integers q_h, p_h, and adds
//      them to the bin's (Q, P, count).  A map of at most OPD_LDS_BINS bins is privatised in LDS (zeroed, filled with LDS integer atomics,
//      its non-zero bins flushed with 64-bit global atomic adds); a larger one is added to global memory directly.  opd_add can aggregate
//      the adds of a wave whose lanes share a bin (BMO_OPD_AGG_ITERS); measured, plain per-lane atomics won and are the default.  Integer
//      adds only: the sums do not depend on their order, which is what makes sweep = single = resident rows bit for bit without a sort.
//   finish  a thread per bin writes opd, weight and raw; the blocks' filled-bin counts, row counts and extrema are folded per configuration
//      (integers, min and max: order-free).
// LDS budget: 20 bytes a bin (int64 Q, int64 P, uint32 count).  OPD_LDS_BINS = 4 096 bins (n <= 64, the Python layer's default) is 80 KiB, two
// workgroups on a CU's 160 KiB: two waves per SIMD, which a pass that spends its time on FP64 arithmetic (the terms and two divisions per row)
// still runs several times faster than the same adds sent to global memory one by one (the flush never sends more global adds
// than the rows would have).  The LDS a launch asks for is its own map's: n = 32 takes 20 KiB and runs at the CU's full 32 waves, n = 45 40 KiB.
#ifndef BMO_OPD_AGG_ITERS
#define BMO_OPD_AGG_ITERS 0  // distinct bins a wave adds by ballot and reduction before the remaining lanes add singly; 0: plain per-lane atomics,
#endif                       // which measured faster on ordered and on shuffled rows (profiles/psf_opd_bench.txt); the tests hold for either
namespace {

constexpr int OPD_LDS_BINS = 4096;
constexpr int OPD_AGG_ITERS = BMO_OPD_AGG_ITERS;
static_assert(OPD_AGG_ITERS >= 0 && OPD_AGG_ITERS <= 8, "OPD_AGG_ITERS: 0 .. 8");

#define OPD_SUM_E(F) ZERN_SUM_D(F) F(mq, SumMax0) F(mp, SumMax0) F(n_bad, SumAdd)
SUM_RECORD(OpdSumE, OPD_SUM_E);
// what pass M and the finish need of configuration c
struct OpdMid {
    double scale_q, scale_p, inv_q, inv_p;  // ldexp(1.0, SH_Q), ldexp(1.0, SH_P), ldexp(1.0, -SH_Q), ldexp(1.0, -SH_P)
    int32_t status, pad;
};

// pass E of work item blockIdx.x
template <int ORDER>
__global__ __launch_bounds__(256) void psf_opd_residual_kernel(const double4* __restrict__ col, const SplitWork* __restrict__ work, const ZernMid* __restrict__ mid,
                                                               const double* __restrict__ coef, OpdSumE* __restrict__ partial) {
    constexpr int J = zern_terms_of(ORDER);
    const SplitWork W = work[blockIdx.x];
    const ZernMid M = mid[W.cfg];
    double cf[J];
#pragma unroll
    for (int j = 0; j < J; ++j) cf[j] = coef[(int64_t)W.cfg * J + j];
    sum_pass_strided(W, partial, [&](OpdSumE& s, int64_t h) {
        const double4 q = col[h];
        const double e = zern_residual_add<ORDER>(s, q, M, cf);
        const double pe = q.x * e;
        const double aq = fabs(pe), ap = fabs(q.x);
        s.mq = aq > s.mq ? aq : s.mq;
        s.mp = ap > s.mp ? ap : s.mp;
        s.n_bad += (isfinite(q.x) && isfinite(pe)) ? 0.0 : 1.0;
    });
}

// sh(M) of include/bmo.h for N <= 2^b rows
__device__ __forceinline__ int opd_shift(double m, int b) {
    if (m == 0.0) return 0;
    const int sh = 60 - b - ilogb(m);
    return sh < -1000 ? -1000 : sh > 1000 ? 1000 : sh;
}

// The info columns of passes A and B come from the Zernike info row zinfo[c] those passes wrote; this writes the rest up to N_BAD, the shifts,
// and mid[c] for pass M and the finish.
struct OpdResidualFinish {
    const int64_t* count;
    const double* zinfo;
    double* info;
    OpdMid* mid;
    __device__ void empty(int32_t c) const {
        double* out = info + (int64_t)c * BMO_OPD_INFO_N;
        for (int q = 0; q < BMO_OPD_INFO_N; ++q) out[q] = knan();
        out[BMO_OPD_N_ROWS] = 0.0;
        out[BMO_OPD_STATUS] = 1.0;
        mid[c] = OpdMid{0.0, 0.0, 0.0, 0.0, 1, 0};
    }
    __device__ void operator()(int32_t c, const OpdSumE& s) const {
        double* out = info + (int64_t)c * BMO_OPD_INFO_N;
        const double* z = zinfo + (int64_t)c * BMO_ZERNIKE_INFO_N;
        for (int q = 0; q <= BMO_ZERNIKE_W_MEAN; ++q) out[q] = z[q];  // the two enums agree up to N_OUT (static_assert below)
        const double rho = z[BMO_ZERNIKE_RHO];
        const int status = (rho == 0.0 || !isfinite(rho)) ? 1 : s.n_bad > 0.0 ? 2 : 0;
        const bool usable = status != 1;
        out[BMO_OPD_STATUS] = (double)status;
        out[BMO_OPD_E_RMS] = usable ? sqrt(s.var / z[BMO_ZERNIKE_S]) : knan();
        out[BMO_OPD_E_LO] = usable ? s.lo : knan();
        out[BMO_OPD_E_HI] = usable ? s.hi : knan();
        out[BMO_OPD_N_OUT] = s.n_out;
        out[BMO_OPD_N_BAD] = s.n_bad;
        const int64_t n = count[c];
        int b = 0;
        while (((int64_t)1 << b) < n) ++b;
        const int sh_q = status == 0 ? opd_shift(s.mq, b) : 0, sh_p = status == 0 ? opd_shift(s.mp, b) : 0;
        out[BMO_OPD_SH_Q] = status == 0 ? (double)sh_q : knan();
        out[BMO_OPD_SH_P] = status == 0 ? (double)sh_p : knan();
        mid[c] = OpdMid{ldexp(1.0, sh_q), ldexp(1.0, sh_p), ldexp(1.0, -sh_q), ldexp(1.0, -sh_p), status, 0};
    }
};
static_assert(BMO_OPD_N_ROWS == (int)BMO_ZERNIKE_N_ROWS && BMO_OPD_STATUS == (int)BMO_ZERNIKE_STATUS && BMO_OPD_S == (int)BMO_ZERNIKE_S &&
                  BMO_OPD_X_REF == (int)BMO_ZERNIKE_X_REF && BMO_OPD_Z_REF == (int)BMO_ZERNIKE_Z_REF && BMO_OPD_U0 == (int)BMO_ZERNIKE_U0 &&
                  BMO_OPD_V0 == (int)BMO_ZERNIKE_V0 && BMO_OPD_RHO == (int)BMO_ZERNIKE_RHO && BMO_OPD_W_MEAN == (int)BMO_ZERNIKE_W_MEAN,
              "the OPD info row begins like the Zernike info row");

// (Q, P, count)[key] += (q, p, 1) for every lane with `live`, called by whole waves in uniform control flow (a lane without a row passes
// live = false).  The first live lane's bin is taken, the lanes that share it are found by ballot, their q and p are summed over the wave
// (integer adds: any tree is exact) and that lane adds the three sums; after OPD_AGG_ITERS such bins the lanes left add singly.
template <class Cnt>
__device__ __forceinline__ void opd_add(unsigned long long* Q, unsigned long long* P, Cnt* N, int32_t key, long long q, long long p, bool live) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int it = 0; it < OPD_AGG_ITERS; ++it) {
        const unsigned long long lm = __ballot(live);
        if (lm == 0) break;  // wave-uniform
        const int first = __ffsll((long long)lm) - 1;
        const int32_t k = __builtin_amdgcn_readlane(key, first);
        const bool match = live && key == k;
        const unsigned long long mm = __ballot(match);
        long long sq = match ? q : 0, sp = match ? p : 0;
        for (int off = 32; off > 0; off >>= 1) {
            sq += __shfl_xor(sq, off);
            sp += __shfl_xor(sp, off);
        }
        if (lane == first) {
            atomicAdd(&Q[k], (unsigned long long)sq);
            atomicAdd(&P[k], (unsigned long long)sp);
            atomicAdd(&N[k], (Cnt)__popcll(mm));
        }
        live = live && !match;
    }
    if (live) {
        atomicAdd(&Q[key], (unsigned long long)q);
        atomicAdd(&P[key], (unsigned long long)p);
        atomicAdd(&N[key], (Cnt)1);
    }
}

// pass M of work item blockIdx.x: its rows binned into (gq, gp, gc)[cfg][n * n].  A configuration of STATUS 1 bins nothing; one of STATUS 2
// counts its rows and adds q = p = 0.
template <int ORDER, bool LDS>
__global__ __launch_bounds__(256) void psf_opd_bin_kernel(const double4* __restrict__ col, const SplitWork* __restrict__ work, const ZernMid* __restrict__ mid,
                                                          const double* __restrict__ coef, const OpdMid* __restrict__ omid, int32_t n,
                                                          unsigned long long* __restrict__ gq, unsigned long long* __restrict__ gp,
                                                          unsigned long long* __restrict__ gc) {
    extern __shared__ unsigned long long opd_lds[];  // LDS: Q [n * n], P [n * n], then the uint32 counts [n * n]
    constexpr int J = zern_terms_of(ORDER);
    const SplitWork W = work[blockIdx.x];
    const OpdMid O = omid[W.cfg];
    if (O.status == 1) return;  // the whole workgroup
    const ZernMid M = mid[W.cfg];
    const int32_t n_bins = n * n;
    unsigned long long *lq = opd_lds, *lp = opd_lds + n_bins;
    uint32_t* lc = (uint32_t*)(opd_lds + 2 * (size_t)n_bins);
    gq += (int64_t)W.cfg * n_bins, gp += (int64_t)W.cfg * n_bins, gc += (int64_t)W.cfg * n_bins;
    if (LDS) {
        for (int32_t b = threadIdx.x; b < n_bins; b += 256) lq[b] = 0, lp[b] = 0, lc[b] = 0;
        __syncthreads();
    }
    double cf[J];
#pragma unroll
    for (int j = 0; j < J; ++j) cf[j] = coef[(int64_t)W.cfg * J + j];
    const double sx = (double)n / 2.0;
    const SpotWindow B{-1.0, 1.0, -1.0, 1.0, sx, sx};
    for (int64_t base = W.h0; base < W.h1; base += 256) {  // workgroup-uniform trips: opd_add needs whole waves
        const int64_t h = base + threadIdx.x;
        int32_t key = -1;
        long long q = 0, p = 0;
        if (h < W.h1) {
            const double4 r = col[h];
            double x, y;
            const double e = zern_residual<ORDER>(r, M, cf, x, y);
            key = spot_bin(x, y, B, n, n);
            if (key >= 0 && O.status == 0) {
                q = (long long)rint((r.x * e) * O.scale_q);
                p = (long long)rint(r.x * O.scale_p);
            }
        }
        if (LDS) opd_add(lq, lp, lc, key, q, p, key >= 0);
        else opd_add(gq, gp, gc, key, q, p, key >= 0);
    }
    if (LDS) {
        __syncthreads();
        for (int32_t b = threadIdx.x; b < n_bins; b += 256) {
            const uint32_t v = lc[b];
            if (v) {
                atomicAdd(&gc[b], (unsigned long long)v);
                if (lq[b]) atomicAdd(&gq[b], lq[b]);
                if (lp[b]) atomicAdd(&gp[b], lp[b]);
            }
        }
    }
}

// what a block of the finish knows of its 256 bins
struct OpdBlockSum {
    unsigned long long filled, rows;
    double lo, hi;  // extrema of the opd that are not NaN (inf, -inf: none)
};

// Bin blockIdx.x * 256 + threadIdx.x of configuration blockIdx.y: opd, weight and raw from the integer sums; the block's sums go to
// part[blockIdx.y][blockIdx.x].
__global__ __launch_bounds__(256) void psf_opd_finish_kernel(const OpdMid* __restrict__ omid, int32_t n_bins, const unsigned long long* __restrict__ gq,
                                                             const unsigned long long* __restrict__ gp, const unsigned long long* __restrict__ gc,
                                                             double* __restrict__ opd, double* __restrict__ weight, long long* __restrict__ raw,
                                                             OpdBlockSum* __restrict__ part) {
    __shared__ OpdBlockSum sh[4];
    const int32_t c = (int32_t)blockIdx.y;
    const OpdMid O = omid[c];
    const int32_t b = (int32_t)(blockIdx.x * 256 + threadIdx.x);
    OpdBlockSum s{0, 0, kinf(), -kinf()};
    if (b < n_bins) {
        const int64_t at = (int64_t)c * n_bins + b;
        const long long Q = (long long)gq[at], P = (long long)gp[at];
        const unsigned long long cnt = gc[at];
        double w = knan(), v = knan();
        if (O.status == 0) {
            w = (double)P * O.inv_p;
            if (cnt != 0 && P != 0) v = ((double)Q * O.inv_q) / w;
        }
        opd[at] = v;
        weight[at] = w;
        if (raw) raw[2 * at] = Q, raw[2 * at + 1] = P;
        s.filled = cnt != 0;
        s.rows = cnt;
        if (v == v) s.lo = v, s.hi = v;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s.filled += __shfl_down(s.filled, off);
        s.rows += __shfl_down(s.rows, off);
        const double lo = __shfl_down(s.lo, off), hi = __shfl_down(s.hi, off);
        s.lo = lo < s.lo ? lo : s.lo;
        s.hi = hi > s.hi ? hi : s.hi;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            s.filled += sh[w].filled, s.rows += sh[w].rows;
            s.lo = sh[w].lo < s.lo ? sh[w].lo : s.lo;
            s.hi = sh[w].hi > s.hi ? sh[w].hi : s.hi;
        }
        part[(int64_t)c * gridDim.x + blockIdx.x] = s;
    }
}

// configuration blockIdx.x: the n_blocks block sums folded into N_OUTSIDE, N_FILLED, MAP_LO and MAP_HI (integers, min and max: any order)
__global__ __launch_bounds__(256) void psf_opd_info_kernel(const int64_t* __restrict__ count, const OpdMid* __restrict__ omid, const OpdBlockSum* __restrict__ part,
                                                           int32_t n_blocks, double* __restrict__ info) {
    __shared__ OpdBlockSum sh[4];
    const int32_t c = (int32_t)blockIdx.x;
    OpdBlockSum s{0, 0, kinf(), -kinf()};
    for (int32_t i = threadIdx.x; i < n_blocks; i += 256) {
        const OpdBlockSum v = part[(int64_t)c * n_blocks + i];
        s.filled += v.filled, s.rows += v.rows;
        s.lo = v.lo < s.lo ? v.lo : s.lo;
        s.hi = v.hi > s.hi ? v.hi : s.hi;
    }
    for (int off = 32; off > 0; off >>= 1) {
        s.filled += __shfl_down(s.filled, off);
        s.rows += __shfl_down(s.rows, off);
        const double lo = __shfl_down(s.lo, off), hi = __shfl_down(s.hi, off);
        s.lo = lo < s.lo ? lo : s.lo;
        s.hi = hi > s.hi ? hi : s.hi;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x != 0 || count[c] == 0) return;  // no rows: answered already
    for (int w = 1; w < 4; ++w) {
        s.filled += sh[w].filled, s.rows += sh[w].rows;
        s.lo = sh[w].lo < s.lo ? sh[w].lo : s.lo;
        s.hi = sh[w].hi > s.hi ? sh[w].hi : s.hi;
    }
    double* out = info + (int64_t)c * BMO_OPD_INFO_N;
    const bool any = omid[c].status == 0 && s.lo <= s.hi;
    out[BMO_OPD_N_OUTSIDE] = (double)(count[c] - (int64_t)s.rows);
    out[BMO_OPD_N_FILLED] = (double)s.filled;
    out[BMO_OPD_MAP_LO] = any ? s.lo + 0.0 : knan();
    out[BMO_OPD_MAP_HI] = any ? s.hi + 0.0 : knan();
}

}  // namespace

// what a slot without rows reads: every configuration like a call with n_hits = 0
static void psf_opd_empty(int32_t n_configs, int64_t n_bins, double* opd, double* weight, int64_t* count, int64_t* raw, double* info) {
    const size_t cells = (size_t)n_configs * (size_t)n_bins;
    std::fill(opd, opd + cells, std::nan(""));
    std::fill(weight, weight + cells, std::nan(""));
    std::fill(count, count + cells, (int64_t)0);
    if (raw) std::fill(raw, raw + 2 * cells, (int64_t)0);
    fill_empty_stats(info, (size_t)n_configs, BMO_OPD_INFO_N);
    for (int32_t c = 0; c < n_configs; ++c) info[(size_t)c * BMO_OPD_INFO_N + BMO_OPD_STATUS] = 1.0;
}

// the arguments both entries check before a device is looked for
static int psf_opd_args(const double* pupil, int32_t n_configs, int32_t order, const double* coef, int32_t n, const char* who) {
    if (n < 1 || n > BMO_OPD_MAX_N) return fail(BMO_ERR_INVALID, std::string(who) + ": n must be 1 .. 4096 bins per axis");
    if (!psf_zernike_args_ok(pupil, n_configs, order))
        return fail(BMO_ERR_INVALID, std::string(who) + ": order must be 0 .. 6, every given pupil (U0, V0, RHO) finite with RHO > 0");
    if (!coef && order != 0) return fail(BMO_ERR_INVALID, std::string(who) + ": coef may be NULL only with order = 0");
    for (int64_t q = 0; coef && q < (int64_t)n_configs * zern_terms_of(order); ++q)
        if (!std::isfinite(coef[q])) return fail(BMO_ERR_INVALID, std::string(who) + ": a given coefficient is not finite");
    if ((double)n_configs * (double)n * (double)n * 24.0 > 4294967296.0)
        return fail(BMO_ERR_LIMIT, std::string(who) + ": the bin arrays of the call would pass 4 GiB");
    return BMO_OK;
}

// The maps of the K configurations from the n_rows device rows `hits` [..][9]: the arguments of psf_zernike_read, coef nullptr (order 0:
// nothing removed) or [K][J]; opd, weight, count [K][n * n], raw nullptr or [K][n * n][2], info [K][BMO_OPD_INFO_N].
static int psf_opd_read(const double* hits, int64_t n_rows, const Ranges& R, const double* origins, const double* e1s, const double* e2s, const double* ref_xz,
                        const double* pupil, int32_t order, const double* coef, int32_t n, double* opd, double* weight, int64_t* count, int64_t* raw, double* info,
                        double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    const int32_t J = zern_terms_of(order);
    const int32_t n_bins = n * n;
    const size_t cells = K * (size_t)n_bins;
    const unsigned n_blocks = (unsigned)((n_bins + 255) / 256);
    if (K > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more configurations than the finish launch holds");
    RowPasses P(R);
    if (int rc = P.items(who)) return rc;
    const std::vector<double> none(K * (size_t)J, 0.0);
    const size_t o_count = P.up.add(R.count), o_pose = P.up.add(psf_poses(K, origins, e1s, e2s)), o_coef = P.up.add(coef ? coef : none.data(), K * (size_t)J);
    const size_t o_ref = ref_xz ? P.up.add(ref_xz, 2 * K) : 0, o_pupil = pupil ? P.up.add(pupil, 3 * K) : 0;
    DevBuf d_zinfo, d_info, d_mid, d_omid, d_col, d_sums, d_maps, d_raw, d_part;
    int rc;
    if ((rc = d_zinfo.alloc(K * BMO_ZERNIKE_INFO_N * 8)) || (rc = d_info.alloc(K * BMO_OPD_INFO_N * 8)) || (rc = d_mid.alloc(K * sizeof(ZernMid))) ||
        (rc = d_omid.alloc(K * sizeof(OpdMid))) || (rc = d_col.alloc((size_t)n_rows * sizeof(double4))) || (rc = d_sums.alloc(3 * cells * 8)) ||
        (rc = d_maps.alloc(2 * cells * 8)) || (raw && (rc = d_raw.alloc(2 * cells * 8))) || (rc = d_part.alloc(K * (size_t)n_blocks * sizeof(OpdBlockSum))) ||
        (rc = P.begin<ZernSumA, ZernSumB, OpdSumE>()))
        return rc;
    const int64_t* d_count = P.up.at<int64_t>(o_count);
    const PsfPose* d_pose = P.up.at<PsfPose>(o_pose);
    const double* d_coef = P.up.at<double>(o_coef);
    const double* d_pupil = pupil ? P.up.at<double>(o_pupil) : (const double*)nullptr;
    double *const g_zinfo = (double*)d_zinfo.p, *const g_info = (double*)d_info.p;
    ZernMid* const g_mid = (ZernMid*)d_mid.p;
    OpdMid* const g_omid = (OpdMid*)d_omid.p;
    double4* const g_col = (double4*)d_col.p;
    unsigned long long *const g_q = (unsigned long long*)d_sums.p, *const g_p = g_q + cells, *const g_c = g_p + cells;
    double *const g_opd = (double*)d_maps.p, *const g_weight = g_opd + cells;
    HIP_TRY(hipMemsetAsync(d_sums.p, 0, 3 * cells * 8, P.st));
    P.pass<ZernSumA>(psf_zernike_sums_kernel, ZernSumsFinish{d_count, d_pose, ref_xz ? P.up.at<double>(o_ref) : (const double*)nullptr, d_pupil, g_zinfo, g_mid}, hits,
                     P.work(), d_pose);
    P.pass<ZernSumB>(psf_zernike_wave_kernel, ZernWaveFinish{d_pupil, g_zinfo, g_mid}, hits, P.work(), d_pose, g_mid, g_col);
    void (*const residual[])(const double4*, const SplitWork*, const ZernMid*, const double*, OpdSumE*) = {
        psf_opd_residual_kernel<0>, psf_opd_residual_kernel<1>, psf_opd_residual_kernel<2>, psf_opd_residual_kernel<3>,
        psf_opd_residual_kernel<4>, psf_opd_residual_kernel<5>, psf_opd_residual_kernel<6>};
    P.pass<OpdSumE>(residual[order], OpdResidualFinish{d_count, g_zinfo, g_info, g_omid}, g_col, P.work(), g_mid, d_coef);
    using BinKernel = void (*)(const double4*, const SplitWork*, const ZernMid*, const double*, const OpdMid*, int32_t, unsigned long long*, unsigned long long*,
                               unsigned long long*);
    static const BinKernel bin_lds[] = {psf_opd_bin_kernel<0, true>, psf_opd_bin_kernel<1, true>, psf_opd_bin_kernel<2, true>, psf_opd_bin_kernel<3, true>,
                                        psf_opd_bin_kernel<4, true>, psf_opd_bin_kernel<5, true>, psf_opd_bin_kernel<6, true>};
    static const BinKernel bin_global[] = {psf_opd_bin_kernel<0, false>, psf_opd_bin_kernel<1, false>, psf_opd_bin_kernel<2, false>, psf_opd_bin_kernel<3, false>,
                                           psf_opd_bin_kernel<4, false>, psf_opd_bin_kernel<5, false>, psf_opd_bin_kernel<6, false>};
    if (P.n_items > 0) {
        const bool lds = n_bins <= OPD_LDS_BINS;
        // more dynamic LDS than a launch gets by default (64 KiB) has to be asked for, once per kernel
        if (lds) HIP_TRY(hipFuncSetAttribute((const void*)bin_lds[order], hipFuncAttributeMaxDynamicSharedMemorySize, OPD_LDS_BINS * 20));
        hipLaunchKernelGGL(lds ? bin_lds[order] : bin_global[order], P.grid, dim3(256), lds ? (size_t)n_bins * 20 : 0, P.st, g_col, P.work(), g_mid, d_coef, g_omid, n, g_q,
                           g_p, g_c);
    }
    hipLaunchKernelGGL(psf_opd_finish_kernel, dim3(n_blocks, (unsigned)K), dim3(256), 0, P.st, g_omid, n_bins, g_q, g_p, g_c, g_opd, g_weight,
                       raw ? (long long*)d_raw.p : (long long*)nullptr, (OpdBlockSum*)d_part.p);
    hipLaunchKernelGGL(psf_opd_info_kernel, dim3((unsigned)K), dim3(256), 0, P.st, d_count, g_omid, (const OpdBlockSum*)d_part.p, (int32_t)n_blocks, g_info);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(info, d_info.p, K * BMO_OPD_INFO_N * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(opd, g_opd, cells * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(weight, g_weight, cells * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, g_c, cells * 8, hipMemcpyDeviceToHost));
    if (raw) HIP_TRY(hipMemcpy(raw, d_raw.p, 2 * cells * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_opd_map(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                               const double* ref_xz, const double* pupil, int32_t order, const double* coef, int32_t n, int32_t device, double* opd, double* weight,
                               int64_t* count, int64_t* raw, double* info, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !opd || !weight || !count || !info || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_opd_map: bad argument (null pointer, n_hits < 0)");
    if (int rc = psf_opd_args(pupil, 1, order, coef, n, "bmo_psf_opd_map")) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_opd_map", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    return psf_opd_read(hits, n_hits, Ranges{{0}, {n_hits}}, origin, e1, e2, ref_xz, pupil, order, coef, n, opd, weight, count, raw, info, kernel_ms, "bmo_psf_opd_map");
}

extern "C" int bmo_psf_opd_map_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                     const double* ref_xz, const double* pupil, int32_t order, const double* coef, int32_t n, double* opd, double* weight,
                                     int64_t* count, int64_t* raw, double* info, double* kernel_ms) {
    if (!res || !origins || !e1s || !e2s || !opd || !weight || !count || !info) return fail(BMO_ERR_INVALID, "bmo_psf_opd_map_sweep: bad argument");
    if (int rc = slot_check("bmo_psf_opd_map_sweep", res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    if (int rc = psf_opd_args(pupil, n_configs, order, coef, n, "bmo_psf_opd_map_sweep")) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_hits = 0
        psf_opd_empty(n_configs, (int64_t)n * n, opd, weight, count, raw, info);
        return BMO_OK;
    }
    Ranges R;
    const double* hits;
    if (int rc = resident_rows("bmo_psf_opd_map_sweep", res, detector, H, n_configs, R, hits)) return rc;
    return psf_opd_read(hits, H, R, origins, e1s, e2s, ref_xz, pupil, order, coef, n, opd, weight, count, raw, info, kernel_ms, "bmo_psf_opd_map_sweep");
}

// ====================================================================================================================
// Through-focus read-out (include/bmo.h "Through-focus read-out"): the PSF of one set of rows on a stack of displaced grids, and the spot
// statistics of the rows propagated to a stack of planes.
//
// The stack.  The split plan, the point blocks and the order of the sum over rows are bmo_psf_intensity's for the same (n_hits, n); a
// workgroup owns 256 grid points, one split and one chunk of MP planes, whose 2 * MP accumulators every lane keeps in registers.  Per row
// and point the lane evaluates the sincos of psf_sum_range once and multiplies it by the row's MP plane factors u = cis(k dot(d_m, dir)).
// The factors do not depend on the point: for every psf_focus_rows(MP) rows of the staged tile the workgroup computes them cooperatively
// (at most 1 024 factors, four per lane) into at most 16 KB of LDS laid out [plane][row] (the lanes that write are consecutive in `row`:
// no bank conflict), and every lane then reads the factor of (plane, row) at the same address (a broadcast read).  18 KB of row tile +
// 16 KB of factors: four workgroups, 16 waves, per CU.  A stack runs as chunks of PSF_FOCUS_MP planes on the grid's z dimension, each of
// which repeats the per-point sincos, and one launch of the next power of two for the planes that are left (MP = 1, 2, 4, 8 ...), so a
// single plane pays for one factor per row and point and not for sixteen.  The partial sums are [item][plane][point], which
// reduce_splits_kernel reads as one configuration of n_planes * n_pts points; a stack whose partial sums would pass 1 GiB runs in several
// passes of whole chunks.
#ifndef BMO_PSF_FOCUS_MP
#define BMO_PSF_FOCUS_MP 16  // planes per full chunk: 8 or 16 (the A/B that chose it: profiles/psf_through_focus_bench.txt)
#endif
namespace {

constexpr int PSF_FOCUS_MP = BMO_PSF_FOCUS_MP;
static_assert(PSF_FOCUS_MP == 8 || PSF_FOCUS_MP == 16, "PSF_FOCUS_MP: 8 or 16");
// rows whose factors are in LDS together for chunks of mp planes: 1 024 factors, at most the tile
constexpr int psf_focus_rows(int mp) { return 1024 / mp < PSF_TILE ? 1024 / mp : PSF_TILE; }

// Rows h0 .. h1 - 1 on planes m_first + blockIdx.z * MP .. of the n_planes displacements `disp` [n_planes][3], summed in row order into row
// blockIdx.y of the partial plane of a pass that starts at plane m_pass and holds pass_planes planes: [item][m - m_pass][pt].  Every lane of
// the workgroup calls it (it syncs).
template <int MP>
__device__ __forceinline__ void psf_focus_sum_chunk(const double* __restrict__ hits, int64_t h0, int64_t h1, const double* __restrict__ xs,
                                                    const double* __restrict__ zs, int32_t n, const d3& origin, const d3& e1, const d3& e2,
                                                    const double* __restrict__ disp, int32_t n_planes, int32_t m_first, int32_t m_pass, int32_t pass_planes,
                                                    double2* __restrict__ partial) {
    constexpr int FR = psf_focus_rows(MP);
    static_assert(PSF_TILE % FR == 0 && (MP * FR) % 256 == 0, "whole factor sub-tiles, every lane computes as many factors");
    __shared__ double tile[PSF_TILE * 9];
    __shared__ double2 fac[MP * FR];
    __shared__ double dsp[MP * 3];
    const int64_t n_pts = (int64_t)n * n;
    const int64_t pt = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = pt < n_pts;
    const int32_t m0 = m_first + (int32_t)blockIdx.z * MP;
    const int mcnt = n_planes - m0 < MP ? n_planes - m0 : MP;  // planes of this chunk; the slots past them run on d = 0 and are not stored
    if ((int)threadIdx.x < MP * 3) dsp[threadIdx.x] = (int)threadIdx.x < mcnt * 3 ? disp[(int64_t)m0 * 3 + threadIdx.x] : 0.0;
    d3 p{0, 0, 0};
    if (live) p = psf_point(origin, e1, e2, xs[(int)(pt % n)], zs[(int)(pt / n)]);
    double re[MP], im[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) re[m] = 0.0, im[m] = 0.0;
    for (int64_t base = h0; base < h1; base += PSF_TILE) {
        const int cnt = (int)(h1 - base < PSF_TILE ? h1 - base : PSF_TILE);
        psf_stage_rows(hits, base, cnt, tile);  // its syncs also publish dsp
        for (int sub = 0; sub < cnt; sub += FR) {
            const int scnt = cnt - sub < FR ? cnt - sub : FR;
            if (sub > 0) __syncthreads();  // the factors of the rows before are read
            for (int q = threadIdx.x; q < MP * FR; q += 256) {
                const int row = q % FR, m = q / FR;
                if (row < scnt) {
                    const double* r = tile + 9 * (sub + row);
                    const double g = (dsp[3 * m] * r[3] + dsp[3 * m + 1] * r[4]) + dsp[3 * m + 2] * r[5];
                    double s, c;
                    sincos(r[8] * g, &s, &c);
                    fac[q] = make_double2(c, s);
                }
            }
            __syncthreads();
            if (live) {
                for (int h = 0; h < scnt; ++h) {
                    const double* r = tile + 9 * (sub + h);
                    const double phase = r[8] * psf_path(p, r);
                    double s, c;
                    sincos(phase, &s, &c);
                    const double t_re = r[7] * c, t_im = r[7] * s;
#pragma unroll
                    for (int m = 0; m < MP; ++m) {
                        const double2 u = fac[m * FR + h];
                        re[m] += t_re * u.x - t_im * u.y;
                        im[m] += t_re * u.y + t_im * u.x;
                    }
                }
            }
        }
    }
    if (!live) return;
    double2* out = partial + ((int64_t)blockIdx.y * pass_planes + (m0 - m_pass)) * n_pts + pt;
#pragma unroll
    for (int m = 0; m < MP; ++m)
        if (m < mcnt) out[(int64_t)m * n_pts] = make_double2(re[m], im[m]);
}

// A launch of one configuration, which every single call is: split blockIdx.y of its n_hits rows, the pose in the kernel arguments
template <int MP>
__global__ __launch_bounds__(256) void psf_focus_accumulate_kernel(const double* __restrict__ hits, int64_t n_hits, int64_t hits_per_split,
                                                                   const double* __restrict__ xs, const double* __restrict__ zs, int32_t n, d3 origin, d3 e1,
                                                                   d3 e2, const double* __restrict__ disp, int32_t n_planes, int32_t m_first,
                                                                   int32_t m_pass, int32_t pass_planes, double2* __restrict__ partial) {
    const int64_t h0 = (int64_t)blockIdx.y * hits_per_split;
    const int64_t h1 = h0 + hits_per_split < n_hits ? h0 + hits_per_split : n_hits;
    psf_focus_sum_chunk<MP>(hits, h0, h1, xs, zs, n, origin, e1, e2, disp, n_planes, m_first, m_pass, pass_planes, partial);
}

// work item w0 + blockIdx.y, on its configuration's axes (xs, zs: [K][n]), pose and displacements (disp: [K][n_planes][3])
template <int MP>
__global__ __launch_bounds__(256) void psf_focus_accumulate_list_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, int64_t w0,
                                                                        const PsfPose* __restrict__ pose, const double* __restrict__ xs,
                                                                        const double* __restrict__ zs, int32_t n, const double* __restrict__ disp,
                                                                        int32_t n_planes, int32_t m_first, int32_t m_pass, int32_t pass_planes,
                                                                        double2* __restrict__ partial) {
    const SplitWork W = work[w0 + blockIdx.y];
    const PsfPose& C = pose[W.cfg];
    psf_focus_sum_chunk<MP>(hits, W.h0, W.h1, xs + (int64_t)W.cfg * n, zs + (int64_t)W.cfg * n, n, C.origin, C.e1, C.e2, disp + (int64_t)W.cfg * n_planes * 3,
                            n_planes, m_first, m_pass, pass_planes, partial);
}

// what becomes of the sum of point i = c * pass_pts + q of a pass over the planes m_pass .. of a sweep's stacks: it goes to
// [c][m_pass + m][pt], q = m * n_pts + pt (`intensity` and `field` start at plane m_pass of configuration 0; cfg_pts = n_planes * n_pts)
struct PsfStackFinish {
    double* intensity;
    double2* field;  // nullptr: not asked for
    int64_t pass_pts, cfg_pts;
    __device__ void operator()(int64_t i, double re, double im) const {
        const int64_t o = i / pass_pts * cfg_pts + i % pass_pts;
        intensity[o] = re * re + im * im;  // abs2
        if (field) field[o] = make_double2(re, im);
    }
};

}  // namespace

// The stack of n_planes planes from the n_hits > 0 device rows `hits`, left on the device: d_int [n_planes][n * n], and d_field likewise when
// want_field.  `timer` runs from the first launch; the caller may queue more behind the stack on stream 0 and stop it again.
static int psf_focus_stack(const double* hits, int64_t n_hits, const double* origin, const double* e1, const double* e2, const double* disp, int32_t n_planes,
                           const double* xs, const double* zs, int32_t n, bool want_field, DevBuf& d_int, DevBuf& d_field, EventTimer& timer, double* kernel_ms) {
    const int64_t n_pts = (int64_t)n * n;
    const unsigned pt_blocks = (unsigned)((n_pts + 255) / 256);
    const size_t n_out = (size_t)n_planes * (size_t)n_pts;
    hipStream_t st = 0;
    const Ranges R{{0}, {n_hits}};
    const SplitPlan plan(R, pt_blocks, n_pts, psf_splits);  // bmo_psf_intensity's splits of these rows on this grid
    const PsfPose pose{d3{origin[0], origin[1], origin[2]}, d3{e1[0], e1[1], e1[2]}, d3{e2[0], e2[1], e2[2]}};
    Packed up;
    const size_t o_cfg = up.add(plan.cfg), o_xs = up.add(xs, (size_t)n), o_zs = up.add(zs, (size_t)n), o_d = up.add(disp, (size_t)n_planes * 3);
    int rc;
    if ((rc = up.upload(st)) || (rc = d_int.alloc(n_out * sizeof(double))) || (want_field && (rc = d_field.alloc(n_out * sizeof(double2))))) return rc;
    // planes per pass: whole chunks, partial sums of at most 1 GiB (one chunk if a single one needs more)
    const int64_t fit = ((int64_t)1 << 30) / (plan.max_nw * n_pts * (int64_t)sizeof(double2)) / PSF_FOCUS_MP * PSF_FOCUS_MP;
    const int32_t per_pass = (int32_t)std::min<int64_t>(std::max<int64_t>(fit, PSF_FOCUS_MP), (int64_t)65535 * PSF_FOCUS_MP);
    for (int32_t m_pass = 0; m_pass < n_planes; m_pass += per_pass) {
        const int32_t pass_planes = std::min(per_pass, n_planes - m_pass);
        auto accumulate = [&](dim3, const SplitPlan::Launch& L, double2* partial) {
            auto launch = [&](auto mp, int32_t m_first, int32_t chunks) {
                hipLaunchKernelGGL(psf_focus_accumulate_kernel<decltype(mp)::value>, dim3(pt_blocks, (unsigned)L.nw, (unsigned)chunks), dim3(256), 0, st, hits, n_hits,
                                   plan.per_split[0], up.at<double>(o_xs), up.at<double>(o_zs), n, pose.origin, pose.e1, pose.e2, up.at<double>(o_d), n_planes, m_first,
                                   m_pass, pass_planes, partial);
            };
            const int32_t full = pass_planes / PSF_FOCUS_MP, rest = pass_planes % PSF_FOCUS_MP, m_rest = m_pass + full * PSF_FOCUS_MP;
            if (full > 0) launch(std::integral_constant<int, PSF_FOCUS_MP>{}, m_pass, full);
            if (rest > 8) launch(std::integral_constant<int, 16>{}, m_rest, 1);  // the slots past the last plane run idle
            else if (rest > 4) launch(std::integral_constant<int, 8>{}, m_rest, 1);
            else if (rest > 2) launch(std::integral_constant<int, 4>{}, m_rest, 1);
            else if (rest > 1) launch(std::integral_constant<int, 2>{}, m_rest, 1);
            else if (rest > 0) launch(std::integral_constant<int, 1>{}, m_rest, 1);
        };
        const PsfFinish finish{(double*)d_int.p + (int64_t)m_pass * n_pts, want_field ? (double2*)d_field.p + (int64_t)m_pass * n_pts : nullptr};
        if ((rc = split_reduce(plan, up.at<SplitCfg>(o_cfg), (int64_t)pass_planes * n_pts, st, timer, kernel_ms, accumulate, finish))) return rc;
    }
    return BMO_OK;
}

// The stack copied to the caller.
static int psf_focus_read(const double* hits, int64_t n_hits, const double* origin, const double* e1, const double* e2, const double* disp, int32_t n_planes,
                          const double* xs, const double* zs, int32_t n, double* out_intensity, double* out_field, double* kernel_ms) {
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    DevBuf d_int, d_field;
    EventTimer timer;
    if (int rc = psf_focus_stack(hits, n_hits, origin, e1, e2, disp, n_planes, xs, zs, n, out_field != nullptr, d_int, d_field, timer, kernel_ms)) return rc;
    HIP_TRY(hipMemcpy(out_intensity, d_int.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    if (out_field) HIP_TRY(hipMemcpy(out_field, d_field.p, n_out * sizeof(double2), hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_through_focus(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                                     const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, int32_t device,
                                     double* out_intensity, double* out_field, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !displacements || !xs || !zs || !out_intensity || n <= 0 || n_planes <= 0 || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_through_focus: bad argument (null pointer, n <= 0, n_planes <= 0, n_hits < 0)");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_through_focus", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    if (n_hits == 0) {
        const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
        std::fill(out_intensity, out_intensity + n_out, 0.0);
        if (out_field) std::fill(out_field, out_field + 2 * n_out, 0.0);
        return BMO_OK;
    }
    return psf_focus_read(hits, n_hits, origin, e1, e2, displacements, n_planes, xs, zs, n, out_intensity, out_field, kernel_ms);
}

// The focus statistics.  The plumbing of the wavefront statistics (rows_plan, work items on the grid's x dimension, tiles of 256 rows staged
// through LDS, lane l reads row l, sum records: the lane / shuffle / wave / split order of the sums), two accumulate passes with a reduce
// each: A the sums and extrema, its reduce leaves the centroids on the device; C the spreads about them.  A workgroup owns one work item and
// one chunk of FOCUS_STAT_MP planes (the grid's y dimension), whose FOCUS_STAT_MP records every lane keeps in registers: the rows are read
// once per pass and chunk.  The partial sums are [plane][item]; sum_reduce_kernel, one workgroup per plane, folds them in split order.
namespace {

constexpr int FOCUS_STAT_MP = 8;

#define FOCUS_SUM_A(F) F(s, SumAdd) F(bad, SumAdd) F(sx, SumAdd) F(sz, SumAdd) F(x_min, SumMin) F(x_max, SumMax) F(z_min, SumMin) F(z_max, SumMax)
#define FOCUS_SUM_C(F) F(hwx, SumMax0) F(hwz, SumMax0) F(sr2, SumAdd) F(r2_max, SumMax0)
SUM_RECORD(FocusSumA, FOCUS_SUM_A);
SUM_RECORD(FocusSumC, FOCUS_SUM_C);
struct FocusFrame {
    d3 origin, e1, e2, axis, nrm;
};

// (x, z) of row r propagated to the plane through o; den = dot(dir, nrm)
__device__ __forceinline__ void focus_local(const double* r, const FocusFrame& F, const d3& o, double den, double& x, double& z) {
    const double s = (((o.x - r[0]) * F.nrm.x + (o.y - r[1]) * F.nrm.y) + (o.z - r[2]) * F.nrm.z) / den;
    const d3 q{r[0] + s * r[3], r[1] + s * r[4], r[2] + s * r[5]};
    x = ((q.x - o.x) * F.e1.x + (q.y - o.y) * F.e1.y) + (q.z - o.z) * F.e1.z;
    z = ((q.x - o.x) * F.e2.x + (q.y - o.y) * F.e2.y) + (q.z - o.z) * F.e2.z;
}
__device__ __forceinline__ d3 focus_origin(const FocusFrame& F, double off) { return d3{F.origin.x + off * F.axis.x, F.origin.y + off * F.axis.y, F.origin.z + off * F.axis.z}; }
__device__ __forceinline__ double focus_den(const double* r, const FocusFrame& F) { return (r[3] * F.nrm.x + r[4] * F.nrm.y) + r[5] * F.nrm.z; }

// pass A of work item W on planes blockIdx.y * FOCUS_STAT_MP .. of the frame F: the record of plane m goes to out[m * stride + index]
__device__ __forceinline__ void focus_sums_item(const double* __restrict__ hits, const SplitWork& W, const FocusFrame& F, const double* __restrict__ offsets,
                                                int32_t n_planes, FocusSumA* __restrict__ out, int64_t stride, int64_t index) {
    constexpr int MP = FOCUS_STAT_MP;
    const int32_t m0 = (int32_t)blockIdx.y * MP;
    const int mcnt = n_planes - m0 < MP ? n_planes - m0 : MP;
    d3 o[MP];
    FocusSumA a[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        o[m] = focus_origin(F, offsets[m0 + (m < mcnt ? m : 0)]);
        a[m] = sum_identity<FocusSumA>();
    }
    rows_staged(hits, W, [&](const double* r, int64_t) {
        const double w = r[7], den = focus_den(r, F);
        a[0].s += w;  // the two sums that every plane shares are kept once
        a[0].bad += den == 0.0 ? 1.0 : 0.0;
#pragma unroll
        for (int m = 0; m < MP; ++m) {
            double x, z;
            focus_local(r, F, o[m], den, x, z);
            a[m].sx += w * x;
            a[m].sz += w * z;
            a[m].x_min = x < a[m].x_min ? x : a[m].x_min;
            a[m].x_max = x > a[m].x_max ? x : a[m].x_max;
            a[m].z_min = z < a[m].z_min ? z : a[m].z_min;
            a[m].z_max = z > a[m].z_max ? z : a[m].z_max;
        }
    });
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        a[m].s = a[0].s, a[m].bad = a[0].bad;
        const FocusSumA v = sum_wg_reduce(a[m]);
        if (threadIdx.x == 0 && m < mcnt) out[(int64_t)(m0 + m) * stride + index] = v;
    }
}
// a call of one configuration: work item blockIdx.x, the frame in the kernel arguments, the records [plane][item]
__global__ __launch_bounds__(256) void psf_focus_sums_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, FocusFrame F,
                                                             const double* __restrict__ offsets, int32_t n_planes, FocusSumA* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    focus_sums_item(hits, W, F, offsets, n_planes, partial, gridDim.x, blockIdx.x);
}
// Work item blockIdx.x of a sweep at its configuration's frame (frames [K]) and offsets ([K][n_planes]); the frame's address is uniform over
// the workgroup (scalar loads).  The records are [configuration][plane][split]: those of (c, m) start at n_planes * first_work + m * n_splits.
__global__ __launch_bounds__(256) void psf_focus_sums_list_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work,
                                                                  const SplitCfg* __restrict__ cfg, const FocusFrame* __restrict__ frames,
                                                                  const double* __restrict__ offsets, int32_t n_planes, FocusSumA* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const SplitCfg C = cfg[W.cfg];
    focus_sums_item(hits, W, frames[W.cfg], offsets + (int64_t)W.cfg * n_planes, n_planes, partial + (int64_t)n_planes * C.first_work, C.n_splits,
                    (int64_t)blockIdx.x - C.first_work);
}

// the sums, the centroid and the extrema go to stats[m], the centroid to mid[m]
struct FocusSumsFinish {
    int64_t n_rows;
    double* stats;
    double2* mid;
    __device__ void empty(int32_t) const {}  // a plane has every work item of the call
    __device__ void operator()(int32_t m, const FocusSumA& a) const {
        double* out = stats + (int64_t)m * BMO_FOCUS_STAT_N;
        out[BMO_FOCUS_STAT_N_ROWS] = (double)n_rows;
        if (a.bad != 0.0) {  // a row parallel to the planes: no statistics
            for (int q = 1; q < BMO_FOCUS_STAT_N; ++q) out[q] = knan();
            mid[m] = make_double2(knan(), knan());
            return;
        }
        const double cx = a.sx / a.s, cz = a.sz / a.s;
        out[BMO_FOCUS_STAT_S] = a.s;
        out[BMO_FOCUS_STAT_CX] = cx;
        out[BMO_FOCUS_STAT_CZ] = cz;
        out[BMO_FOCUS_STAT_X_MIN] = a.x_min;
        out[BMO_FOCUS_STAT_X_MAX] = a.x_max;
        out[BMO_FOCUS_STAT_Z_MIN] = a.z_min;
        out[BMO_FOCUS_STAT_Z_MAX] = a.z_max;
        mid[m] = make_double2(cx, cz);
    }
};
// the same for range r = c * n_planes + m of a sweep: stats [K][n_planes][..], mid [K][n_planes], count [K] the rows of every configuration
struct FocusSumsListFinish {
    const int64_t* count;
    int32_t n_planes;
    double* stats;
    double2* mid;
    __device__ void empty(int32_t) const {}  // a configuration without rows: the host fills its statistics as the single call does
    __device__ void operator()(int32_t r, const FocusSumA& a) const { FocusSumsFinish{count[r / n_planes], stats, mid}(r, a); }
};

// pass C of work item W on planes blockIdx.y * FOCUS_STAT_MP .. of the frame F, about the centroids mid[m]: the record of plane m goes to
// out[m * stride + index]
__device__ __forceinline__ void focus_spread_item(const double* __restrict__ hits, const SplitWork& W, const FocusFrame& F, const double* __restrict__ offsets,
                                                  int32_t n_planes, const double2* __restrict__ mid, FocusSumC* __restrict__ out, int64_t stride,
                                                  int64_t index) {
    constexpr int MP = FOCUS_STAT_MP;
    const int32_t m0 = (int32_t)blockIdx.y * MP;
    const int mcnt = n_planes - m0 < MP ? n_planes - m0 : MP;
    d3 o[MP];
    double2 c[MP];
    FocusSumC v[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int32_t mm = m0 + (m < mcnt ? m : 0);
        o[m] = focus_origin(F, offsets[mm]);
        c[m] = mid[mm];
        v[m] = sum_identity<FocusSumC>();
    }
    rows_staged(hits, W, [&](const double* r, int64_t) {
        const double w = r[7], den = focus_den(r, F);
#pragma unroll
        for (int m = 0; m < MP; ++m) {
            double x, z;
            focus_local(r, F, o[m], den, x, z);
            const double ax = x - c[m].x, az = z - c[m].y;
            const double fx = fabs(ax), fz = fabs(az);
            const double r2 = ax * ax + az * az;
            v[m].hwx = fx > v[m].hwx ? fx : v[m].hwx;
            v[m].hwz = fz > v[m].hwz ? fz : v[m].hwz;
            v[m].sr2 += w * r2;
            v[m].r2_max = r2 > v[m].r2_max ? r2 : v[m].r2_max;
        }
    });
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const FocusSumC s = sum_wg_reduce(v[m]);
        if (threadIdx.x == 0 && m < mcnt) out[(int64_t)(m0 + m) * stride + index] = s;
    }
}
__global__ __launch_bounds__(256) void psf_focus_spread_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, FocusFrame F,
                                                               const double* __restrict__ offsets, int32_t n_planes, const double2* __restrict__ mid,
                                                               FocusSumC* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    focus_spread_item(hits, W, F, offsets, n_planes, mid, partial, gridDim.x, blockIdx.x);
}
// the list form, laid out as psf_focus_sums_list_kernel's records; mid [K][n_planes]
__global__ __launch_bounds__(256) void psf_focus_spread_list_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work,
                                                                    const SplitCfg* __restrict__ cfg, const FocusFrame* __restrict__ frames,
                                                                    const double* __restrict__ offsets, int32_t n_planes, const double2* __restrict__ mid,
                                                                    FocusSumC* __restrict__ partial) {
    const SplitWork W = work[blockIdx.x];
    const SplitCfg C = cfg[W.cfg];
    focus_spread_item(hits, W, frames[W.cfg], offsets + (int64_t)W.cfg * n_planes, n_planes, mid + (int64_t)W.cfg * n_planes,
                      partial + (int64_t)n_planes * C.first_work, C.n_splits, (int64_t)blockIdx.x - C.first_work);
}

struct FocusSpreadFinish {
    double* stats;
    __device__ void empty(int32_t) const {}  // a plane has every work item of the call
    __device__ void operator()(int32_t m, const FocusSumC& v) const {
        double* out = stats + (int64_t)m * BMO_FOCUS_STAT_N;
        const double s = out[BMO_FOCUS_STAT_S];
        if (s != s) {  // no statistics: a row parallel to the planes, or a NaN proj (then pass A left these four unwritten)
            out[BMO_FOCUS_STAT_HWX] = out[BMO_FOCUS_STAT_HWZ] = out[BMO_FOCUS_STAT_RMS_R] = out[BMO_FOCUS_STAT_MAX_R] = knan();
            return;
        }
        out[BMO_FOCUS_STAT_HWX] = v.hwx;
        out[BMO_FOCUS_STAT_HWZ] = v.hwz;
        out[BMO_FOCUS_STAT_RMS_R] = sqrt(v.sr2 / s);
        out[BMO_FOCUS_STAT_MAX_R] = sqrt(v.r2_max);
    }
};

}  // namespace

// the frame of the planes of a detector pose moved along `axis`: nrm = e1 x e2
static FocusFrame focus_frame(const double* origin, const double* e1, const double* e2, const double* axis) {
    FocusFrame F{d3{origin[0], origin[1], origin[2]}, d3{e1[0], e1[1], e1[2]}, d3{e2[0], e2[1], e2[2]}, d3{axis[0], axis[1], axis[2]}, d3{0, 0, 0}};
    F.nrm = d3{F.e1.y * F.e2.z - F.e1.z * F.e2.y, F.e1.z * F.e2.x - F.e1.x * F.e2.z, F.e1.x * F.e2.y - F.e1.y * F.e2.x};
    return F;
}

// The statistics [n_planes][BMO_FOCUS_STAT_N] of the n_hits > 0 device rows `hits` [..][9] on the planes at offsets[m] * axis.
static int psf_focus_stats_read(const double* hits, int64_t n_hits, const double* origin, const double* e1, const double* e2, const double* axis, const double* offsets,
                                int32_t n_planes, double* stats, double* kernel_ms, const char* who) {
    RowPasses P(Ranges{{0}, {n_hits}});
    if (int rc = P.items(who)) return rc;
    const FocusFrame F = focus_frame(origin, e1, e2, axis);
    const unsigned chunks = (unsigned)((n_planes + FOCUS_STAT_MP - 1) / FOCUS_STAT_MP);
    if (chunks > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more planes than one launch holds");
    // the partial sums are [plane][item]: to the reduces a plane is a range of n_items records like a configuration's
    P.ranges.resize((size_t)n_planes);
    for (int32_t m = 0; m < n_planes; ++m) P.ranges[(size_t)m] = SplitCfg{(int64_t)m * P.n_items, (int32_t)P.n_items, 0};
    const size_t o_off = P.up.add(offsets, (size_t)n_planes);
    DevBuf d_stats, d_mid;
    int rc;
    if ((rc = d_stats.alloc((size_t)n_planes * BMO_FOCUS_STAT_N * 8)) || (rc = d_mid.alloc((size_t)n_planes * sizeof(double2))) || (rc = P.begin<FocusSumA, FocusSumC>()))
        return rc;
    P.grid.y = chunks;  // a workgroup per work item and chunk of planes
    const double* d_off = P.up.at<double>(o_off);
    double* const g_stats = (double*)d_stats.p;
    double2* const g_mid = (double2*)d_mid.p;
    P.pass<FocusSumA>(psf_focus_sums_kernel, FocusSumsFinish{n_hits, g_stats, g_mid}, hits, P.work(), F, d_off, n_planes);
    P.pass<FocusSumC>(psf_focus_spread_kernel, FocusSpreadFinish{g_stats}, hits, P.work(), F, d_off, n_planes, g_mid);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(stats, g_stats, (size_t)n_planes * BMO_FOCUS_STAT_N * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_focus_stats(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                                   const double axis[3], const double* offsets, int32_t n_planes, int32_t device, double* stats, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !axis || !offsets || !stats || n_planes <= 0 || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_focus_stats: bad argument (null pointer, n_planes <= 0, n_hits < 0)");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_focus_stats", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    if (n_hits == 0) {
        fill_empty_stats(stats, (size_t)n_planes, BMO_FOCUS_STAT_N);
        return BMO_OK;
    }
    return psf_focus_stats_read(hits, n_hits, origin, e1, e2, axis, offsets, n_planes, stats, kernel_ms, "bmo_psf_focus_stats");
}

// ====================================================================================================================
// MTF read-out (include/bmo.h "MTF read-out"): the transfer function T(f) = sum w cis(-2 pi (fx x + fz z)) of the rows propagated to a stack
// of planes (geometric), and of the images of the through-focus stack (diffraction).
//
// Geometric.  The PSF kernel's shape with a (plane, frequency) pair for a point: a workgroup owns one split of the rows (the splits of
// spot_splits), one chunk of MP planes and 256 / MP frequencies; lane l holds the sum of pair (l / (256 / MP), l % (256 / MP)) of them.  Per
// staged tile of 256 rows lane r propagates row r to the chunk's planes (focus_local: one division per row and plane, not per pair) and
// writes (x - cx_m, z - cz_m) to LDS laid out [plane][row] (consecutive lanes, consecutive addresses); every lane then walks the tile, the
// lanes of a plane reading one address (broadcast reads).  18 KB of row tile + MP * 4 KB: 50 KB at MP = 8, three workgroups per CU.  The
// sum of a pair runs over the rows of a split in row order and the splits are folded in split order, whatever the chunking: the value
// does not depend on the planes and frequencies asked for along with it.  S and the count of rows parallel to the planes are summed in the
// order of the focus statistics (lane r adds the rows it propagates; sum_wg_reduce; sum_reduce_kernel): S equals BMO_FOCUS_STAT_S.
namespace {

constexpr int GEO_OTF_MP = 8;  // planes per chunk of a stack; a stack of fewer planes runs the next power of two

#define GEO_OTF_SUM(F) F(s, SumAdd) F(bad, SumAdd)
SUM_RECORD(GeoOtfSum, GEO_OTF_SUM);

// Work item W of the rows on planes blockIdx.z * MP .. of the frame F, frequencies blockIdx.x * (256 / MP) ..: the item's sums go to row
// blockIdx.y of `partial` [item][plane][freq], its record (from the workgroups of the first frequency block and chunk) to sums[item].
// Every lane calls it (it syncs).
template <int MP>
__device__ __forceinline__ void geo_otf_item(const double* __restrict__ hits, const SplitWork& W, const FocusFrame& F, const double* __restrict__ offsets,
                                             const double2* __restrict__ centers, int32_t n_planes, const double2* __restrict__ freqs, int32_t n_freqs,
                                             double2* __restrict__ partial, GeoOtfSum* __restrict__ sums, int64_t item) {
    constexpr int FB = 256 / MP;
    static_assert(MP >= 1 && MP <= 8 && 256 % MP == 0, "a chunk of planes divides the workgroup");
    __shared__ double tile[PSF_TILE * 9];
    __shared__ double2 xz[MP * PSF_TILE];
    const int32_t m0 = (int32_t)blockIdx.z * MP;
    const int mcnt = n_planes - m0 < MP ? n_planes - m0 : MP;  // planes of this chunk; the slots past them repeat its first and are not stored
    d3 o[MP];
    double2 c[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int32_t mm = m0 + (m < mcnt ? m : 0);
        o[m] = focus_origin(F, offsets[mm]);
        c[m] = centers ? centers[mm] : make_double2(0.0, 0.0);
    }
    const int ml = (int)threadIdx.x / FB;
    const int32_t f = (int32_t)blockIdx.x * FB + (int)threadIdx.x % FB;
    const bool live = ml < mcnt && f < n_freqs;
    const double2 fq = live ? freqs[f] : make_double2(0.0, 0.0);
    GeoOtfSum a = sum_identity<GeoOtfSum>();
    double re = 0.0, im = 0.0;
    for (int64_t base = W.h0; base < W.h1; base += PSF_TILE) {
        const int cnt = (int)(W.h1 - base < PSF_TILE ? W.h1 - base : PSF_TILE);
        psf_stage_rows(hits, base, cnt, tile);  // its first sync: the walk over the tile before is done
        if ((int)threadIdx.x < cnt) {
            const double* r = tile + 9 * threadIdx.x;
            const double den = focus_den(r, F);
            a.s += r[7];
            a.bad += den == 0.0 ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                double x, z;
                focus_local(r, F, o[m], den, x, z);
                xz[m * PSF_TILE + threadIdx.x] = make_double2(x - c[m].x, z - c[m].y);
            }
        }
        __syncthreads();
        if (live) {
            const double2* p = xz + ml * PSF_TILE;
            for (int h = 0; h < cnt; ++h) {
                const double w = tile[9 * h + 7];
                const double arg = fq.x * p[h].x + fq.y * p[h].y;
                double s, cs;
                sincospi(-2.0 * arg, &s, &cs);
                re += w * cs;
                im += w * s;
            }
        }
    }
    if (live) partial[((int64_t)blockIdx.y * n_planes + (m0 + ml)) * n_freqs + f] = make_double2(re, im);
    if (blockIdx.x == 0 && blockIdx.z == 0) {  // uniform over the workgroup: one record per work item
        a = sum_wg_reduce(a);
        if (threadIdx.x == 0) sums[item] = a;
    }
}
// split blockIdx.y (work item) of the rows of one configuration, the frame in the kernel arguments; partial: [item][plane][freq]
template <int MP>
__global__ __launch_bounds__(256) void psf_geo_otf_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, FocusFrame F,
                                                          const double* __restrict__ offsets, const double2* __restrict__ centers, int32_t n_planes,
                                                          const double2* __restrict__ freqs, int32_t n_freqs, double2* __restrict__ partial,
                                                          GeoOtfSum* __restrict__ sums) {
    const SplitWork W = work[blockIdx.y];
    geo_otf_item<MP>(hits, W, F, offsets, centers, n_planes, freqs, n_freqs, partial, sums, blockIdx.y);
}
// Work item w0 + blockIdx.y of a sweep at its configuration's frame (frames [K]), offsets ([K][n_planes]) and centres (nullptr or
// [K][n_planes]); all configurations share the frequencies.  partial: [item - w0][plane][freq]; sums: one record per item of the sweep.
template <int MP>
__global__ __launch_bounds__(256) void psf_geo_otf_list_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, int64_t w0,
                                                               const FocusFrame* __restrict__ frames, const double* __restrict__ offsets,
                                                               const double2* __restrict__ centers, int32_t n_planes, const double2* __restrict__ freqs,
                                                               int32_t n_freqs, double2* __restrict__ partial, GeoOtfSum* __restrict__ sums) {
    const SplitWork W = work[w0 + blockIdx.y];
    geo_otf_item<MP>(hits, W, frames[W.cfg], offsets + (int64_t)W.cfg * n_planes, centers ? centers + (int64_t)W.cfg * n_planes : nullptr, n_planes, freqs,
                     n_freqs, partial, sums, w0 + blockIdx.y);
}

// S of the call, NaN when a row runs parallel to the planes
struct GeoOtfSumFinish {
    double* s;
    __device__ void empty(int32_t) const {}  // a call with rows has work items
    __device__ void operator()(int32_t, const GeoOtfSum& a) const { *s = a.bad != 0.0 ? knan() : a.s; }
};
// S of every configuration of a sweep: s [K]; 0 for a configuration without rows
struct GeoOtfSumListFinish {
    double* s;
    __device__ void empty(int32_t c) const { s[c] = 0.0; }
    __device__ void operator()(int32_t c, const GeoOtfSum& a) const { GeoOtfSumFinish{s + c}(c, a); }
};

// what becomes of the folded sum (re, im) of pair q = plane * n_freqs + frequency of a call whose rows sum to S: otf, mtf and, from the
// pairs of frequency 0, sums
__device__ __forceinline__ void geo_otf_finish(int64_t q, double re, double im, double S, int32_t n_freqs, double2* __restrict__ otf, double* __restrict__ mtf,
                                               double* __restrict__ sums) {
    if (S != S) re = im = knan();  // a row parallel to the planes (or a NaN proj): no transfer function
    otf[q] = make_double2(re, im);
    mtf[q] = sqrt(re * re + im * im) / S;
    if (q % n_freqs == 0) sums[q / n_freqs] = S;
}
// pair (plane, frequency) = blockIdx.x * 256 + threadIdx.x: its partial sums folded in split order
__global__ void psf_geo_otf_reduce_kernel(const double2* __restrict__ partial, int32_t n_splits, int64_t n_pairs, int32_t n_freqs, const double* __restrict__ s_all,
                                          double2* __restrict__ otf, double* __restrict__ mtf, double* __restrict__ sums) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    double re = 0.0, im = 0.0;
    for (int32_t s = 0; s < n_splits; ++s) {
        const double2 v = partial[(int64_t)s * n_pairs + q];
        re += v.x;
        im += v.y;
    }
    geo_otf_finish(q, re, im, *s_all, n_freqs, otf, mtf, sums);
}
// the same pair of configuration c0 + blockIdx.y of a sweep: its own splits (partial rows first_work - w0 ...) folded in split order;
// otf, mtf [K][n_pairs], sums [K][n_planes], s_all [K]
__global__ void psf_geo_otf_reduce_list_kernel(const SplitCfg* __restrict__ cfg, int32_t c0, int64_t w0, const double2* __restrict__ partial, int64_t n_pairs,
                                               int32_t n_freqs, const double* __restrict__ s_all, double2* __restrict__ otf, double* __restrict__ mtf,
                                               double* __restrict__ sums) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const int32_t c = c0 + (int32_t)blockIdx.y;
    const SplitCfg C = cfg[c];
    double re = 0.0, im = 0.0;
    for (int32_t s = 0; s < C.n_splits; ++s) {
        const double2 v = partial[(C.first_work - w0 + s) * n_pairs + q];
        re += v.x;
        im += v.y;
    }
    geo_otf_finish(q, re, im, s_all[c], n_freqs, otf + (int64_t)c * n_pairs, mtf + (int64_t)c * n_pairs, sums + (int64_t)c * (n_pairs / n_freqs));
}

// Diffraction: the transform of the stack's images where they lie, separable.  Thread (plane m, slot f, row j) sums image row j against the
// x factors of frequency f; slot n_freqs has the factor (1, 0), whose transform is the plane's sum.
// planes_per_axes > 0: that many consecutive images share the axis at xs + (m / planes_per_axes) * n (the stack of one configuration of a
// sweep); 0: every image is on xs
__device__ __forceinline__ void otf_rows_thread(const double* __restrict__ img, const double* __restrict__ xs, int32_t planes_per_axes, int32_t n,
                                                const double2* __restrict__ freqs, int32_t n_freqs, int64_t n_threads, double2* __restrict__ rowsum) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;  // n_planes * (n_freqs + 1) * n
    const int32_t j = (int32_t)(t % n), f = (int32_t)(t / n % (n_freqs + 1));
    const int64_t m = t / n / (n_freqs + 1);
    const double* row = img + (m * n + j) * n;
    if (planes_per_axes > 0) xs += m / planes_per_axes * n;
    double re = 0.0, im = 0.0;
    if (f == n_freqs) {
        for (int32_t i = 0; i < n; ++i) {
            re += row[i] * 1.0;
            im += row[i] * 0.0;
        }
    } else {
        const double fx = freqs[f].x;
        for (int32_t i = 0; i < n; ++i) {
            double s, c;
            sincospi(-2.0 * (fx * xs[i]), &s, &c);
            re += row[i] * c;
            im += row[i] * s;
        }
    }
    rowsum[t] = make_double2(re, im);  // [m][f][j]
}
__global__ void psf_otf_rows_kernel(const double* __restrict__ img, const double* __restrict__ xs, int32_t n, const double2* __restrict__ freqs, int32_t n_freqs,
                                    int64_t n_threads, double2* __restrict__ rowsum) {
    otf_rows_thread(img, xs, 0, n, freqs, n_freqs, n_threads, rowsum);
}
// the K * n_planes images of a sweep's stacks, each against its configuration's axis (xs: [K][n])
__global__ void psf_otf_rows_list_kernel(const double* __restrict__ img, const double* __restrict__ xs, int32_t n_planes, int32_t n,
                                         const double2* __restrict__ freqs, int32_t n_freqs, int64_t n_threads, double2* __restrict__ rowsum) {
    otf_rows_thread(img, xs, n_planes, n, freqs, n_freqs, n_threads, rowsum);
}

// thread (plane m, frequency f): the row sums against the z factors, j ascending; the plane's sum the same way from slot n_freqs
// (planes_per_axes: as in otf_rows_thread, for zs)
__device__ __forceinline__ void otf_cols_thread(const double2* __restrict__ rowsum, const double* __restrict__ zs, int32_t planes_per_axes, int32_t n,
                                                const double2* __restrict__ freqs, int32_t n_freqs, int64_t n_pairs, double2* __restrict__ otf,
                                                double* __restrict__ mtf, double* __restrict__ sums) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const int64_t m = q / n_freqs;
    const int32_t f = (int32_t)(q % n_freqs);
    if (planes_per_axes > 0) zs += m / planes_per_axes * n;
    const double2* r = rowsum + (m * (n_freqs + 1) + f) * n;
    const double2* r1 = rowsum + (m * (n_freqs + 1) + n_freqs) * n;
    const double fz = freqs[f].y;
    double re = 0.0, im = 0.0, S = 0.0;
    for (int32_t j = 0; j < n; ++j) {
        double s, c;
        sincospi(-2.0 * (fz * zs[j]), &s, &c);
        re += r[j].x * c - r[j].y * s;
        im += r[j].x * s + r[j].y * c;
        S += r1[j].x * 1.0 - r1[j].y * 0.0;
    }
    otf[q] = make_double2(re, im);
    mtf[q] = sqrt(re * re + im * im) / S;
    if (f == 0) sums[m] = S;
}
__global__ void psf_otf_cols_kernel(const double2* __restrict__ rowsum, const double* __restrict__ zs, int32_t n, const double2* __restrict__ freqs, int32_t n_freqs,
                                    int64_t n_pairs, double2* __restrict__ otf, double* __restrict__ mtf, double* __restrict__ sums) {
    otf_cols_thread(rowsum, zs, 0, n, freqs, n_freqs, n_pairs, otf, mtf, sums);
}
__global__ void psf_otf_cols_list_kernel(const double2* __restrict__ rowsum, const double* __restrict__ zs, int32_t n_planes, int32_t n,
                                         const double2* __restrict__ freqs, int32_t n_freqs, int64_t n_pairs, double2* __restrict__ otf, double* __restrict__ mtf,
                                         double* __restrict__ sums) {
    otf_cols_thread(rowsum, zs, n_planes, n, freqs, n_freqs, n_pairs, otf, mtf, sums);
}

}  // namespace

// what the two MTF entries refuse of their frequencies
static bool otf_freqs_ok(const double* freqs, int32_t n_freqs) {
    for (int64_t q = 0; q < 2 * (int64_t)n_freqs; ++q)
        if (!std::isfinite(freqs[q])) return false;
    return true;
}
// what a call without rows reads: zeros, and NaN (0 / 0) in mtf
static void otf_fill_empty(size_t n_pairs, size_t n_planes, double* otf, double* mtf, double* sums) {
    std::fill(otf, otf + 2 * n_pairs, 0.0);
    std::fill(mtf, mtf + n_pairs, std::nan(""));
    std::fill(sums, sums + n_planes, 0.0);
}

// The geometric transfer function of the n_hits > 0 device rows `hits` [..][9].
static int psf_geo_otf_read(const double* hits, int64_t n_hits, const double* origin, const double* e1, const double* e2, const double* axis, const double* offsets,
                            const double* centers, int32_t n_planes, const double* freqs, int32_t n_freqs, double* otf, double* mtf, double* sums, double* kernel_ms,
                            const char* who) {
    RowPasses P(Ranges{{0}, {n_hits}});  // the plan, the upload and the reduce of the statistics passes: S is one
    if (int rc = P.items(who)) return rc;
    const FocusFrame F = focus_frame(origin, e1, e2, axis);
    int mp = 1;
    while (mp < GEO_OTF_MP && mp < n_planes) mp *= 2;
    const unsigned chunks = (unsigned)((n_planes + mp - 1) / mp), f_blocks = (unsigned)(((int64_t)n_freqs + 256 / mp - 1) / (256 / mp));
    const int64_t n_pairs = (int64_t)n_planes * n_freqs;
    if (chunks > 65535 || P.n_items > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more planes than one launch holds");
    // a pair's value does not depend on the pairs asked for along with it: a caller with more of them splits the call
    if ((int64_t)P.n_items * n_pairs > ((int64_t)1 << 32) / (int64_t)sizeof(double2))
        return fail(BMO_ERR_LIMIT, std::string(who) + ": the partial sums of n_planes * n_freqs pairs pass 4 GiB; ask for them in several calls");
    const size_t o_off = P.up.add(offsets, (size_t)n_planes), o_freq = P.up.add(freqs, (size_t)n_freqs * 2);
    const size_t o_cen = centers ? P.up.add(centers, (size_t)n_planes * 2) : 0;
    DevBuf d_partial, d_s, d_otf, d_mtf, d_sums;
    int rc;
    if ((rc = d_partial.alloc((size_t)P.n_items * (size_t)n_pairs * sizeof(double2))) || (rc = d_s.alloc(8)) || (rc = d_otf.alloc((size_t)n_pairs * sizeof(double2))) ||
        (rc = d_mtf.alloc((size_t)n_pairs * 8)) || (rc = d_sums.alloc((size_t)n_planes * 8)) || (rc = P.begin<GeoOtfSum>()))
        return rc;
    const double2* d_cen = centers ? P.up.at<double2>(o_cen) : nullptr;
    auto launch = [&](auto MP) {
        hipLaunchKernelGGL(psf_geo_otf_kernel<decltype(MP)::value>, dim3(f_blocks, P.n_items, chunks), dim3(256), 0, P.st, hits, P.work(), F, P.up.at<double>(o_off), d_cen,
                           n_planes, P.up.at<double2>(o_freq), n_freqs, (double2*)d_partial.p, (GeoOtfSum*)P.records.p);
    };
    if (mp == 1) launch(std::integral_constant<int, 1>{});
    else if (mp == 2) launch(std::integral_constant<int, 2>{});
    else if (mp == 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, GEO_OTF_MP>{});
    sum_reduce<GeoOtfSum>(1u, P.st, P.cfg(), P.records, GeoOtfSumFinish{(double*)d_s.p});
    hipLaunchKernelGGL(psf_geo_otf_reduce_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, P.st, (const double2*)d_partial.p, (int32_t)P.n_items, n_pairs, n_freqs,
                       (const double*)d_s.p, (double2*)d_otf.p, (double*)d_mtf.p, (double*)d_sums.p);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(otf, d_otf.p, (size_t)n_pairs * sizeof(double2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mtf, d_mtf.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_geo_otf(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                               const double axis[3], const double* offsets, const double* centers, int32_t n_planes, const double* freqs, int32_t n_freqs, int32_t device,
                               double* otf, double* mtf, double* sums, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !axis || !offsets || !freqs || !otf || !mtf || !sums || n_planes <= 0 || n_freqs <= 0 || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_geo_otf: bad argument (null pointer, n_planes <= 0, n_freqs <= 0, n_hits < 0)");
    if (!otf_freqs_ok(freqs, n_freqs)) return fail(BMO_ERR_INVALID, "bmo_psf_geo_otf: a frequency is not finite");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_geo_otf", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    if (n_hits == 0) {
        otf_fill_empty((size_t)n_planes * (size_t)n_freqs, (size_t)n_planes, otf, mtf, sums);
        return BMO_OK;
    }
    return psf_geo_otf_read(hits, n_hits, origin, e1, e2, axis, offsets, centers, n_planes, freqs, n_freqs, otf, mtf, sums, kernel_ms, "bmo_psf_geo_otf");
}

extern "C" int bmo_psf_otf(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                           const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* freqs, int32_t n_freqs,
                           int32_t device, double* otf, double* mtf, double* sums, double* out_intensity, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !displacements || !xs || !zs || !freqs || !otf || !mtf || !sums || n <= 0 || n_planes <= 0 || n_freqs <= 0 || n_hits < 0 ||
        (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_otf: bad argument (null pointer, n <= 0, n_planes <= 0, n_freqs <= 0, n_hits < 0)");
    if (!otf_freqs_ok(freqs, n_freqs)) return fail(BMO_ERR_INVALID, "bmo_psf_otf: a frequency is not finite");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_otf", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    const int64_t n_pairs = (int64_t)n_planes * n_freqs;
    if (n_hits == 0) {
        otf_fill_empty((size_t)n_pairs, (size_t)n_planes, otf, mtf, sums);
        if (out_intensity) std::fill(out_intensity, out_intensity + n_out, 0.0);
        return BMO_OK;
    }
    const int64_t n_rowsums = (int64_t)n_planes * (n_freqs + 1) * n;
    if ((n_rowsums + 255) / 256 > (int64_t)0x7fffffff) return fail(BMO_ERR_LIMIT, "bmo_psf_otf: more row sums than one launch holds");
    hipStream_t st = 0;
    DevBuf d_int, d_field, d_rowsum, d_otf, d_mtf, d_sums;
    Packed up;
    const size_t o_xs = up.add(xs, (size_t)n), o_zs = up.add(zs, (size_t)n), o_freq = up.add(freqs, (size_t)n_freqs * 2);
    int rc;
    if ((rc = up.upload(st)) || (rc = d_rowsum.alloc((size_t)n_rowsums * sizeof(double2))) || (rc = d_otf.alloc((size_t)n_pairs * sizeof(double2))) ||
        (rc = d_mtf.alloc((size_t)n_pairs * 8)) || (rc = d_sums.alloc((size_t)n_planes * 8)))
        return rc;
    EventTimer timer;
    if ((rc = psf_focus_stack(hits, n_hits, origin, e1, e2, displacements, n_planes, xs, zs, n, false, d_int, d_field, timer, kernel_ms))) return rc;
    hipLaunchKernelGGL(psf_otf_rows_kernel, dim3((unsigned)((n_rowsums + 255) / 256)), dim3(256), 0, st, (const double*)d_int.p, up.at<double>(o_xs), n,
                       up.at<double2>(o_freq), n_freqs, n_rowsums, (double2*)d_rowsum.p);
    hipLaunchKernelGGL(psf_otf_cols_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, (const double2*)d_rowsum.p, up.at<double>(o_zs), n,
                       up.at<double2>(o_freq), n_freqs, n_pairs, (double2*)d_otf.p, (double*)d_mtf.p, (double*)d_sums.p);
    if ((rc = timer.stop(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(otf, d_otf.p, (size_t)n_pairs * sizeof(double2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mtf, d_mtf.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    if (out_intensity) HIP_TRY(hipMemcpy(out_intensity, d_int.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return BMO_OK;
}

// the resident PSF rows of slot `detector`, for the single-call read-outs that take a device pointer: bmo_result_device_hits with the checks
// of the _sweep forms
extern "C" int bmo_result_psf_rows(bmo_trace_result* res, int32_t detector, const double** data, int64_t* count, int32_t* device) {
    if (!res || !data || !count) return fail(BMO_ERR_INVALID, "bmo_result_psf_rows: bad argument");
    if (int rc = slot_check("bmo_result_psf_rows", res, detector, BMO_OBJ_PSFDETECTOR, true, -1)) return rc;
    if (res->n_configs > 0) return fail(BMO_ERR_INVALID, "bmo_result_psf_rows: a sweep result holds the rows of several configurations");
    *count = res->det_count[detector];
    *data = res->det_data.p ? (const double*)res->det_data.p + 9 * res->det_offset[detector] : nullptr;
    if (device) *device = res->device;
    return BMO_OK;
}

// ====================================================================================================================
// Through-focus and MTF read-out of sweeps (include/bmo_sweep_readout.h): the four read-outs above for every configuration of a sweep, from
// the rows resident in the result, in list-form launches that run all configurations' work items in one grid.  Configuration c is split
// as a single call with its row count splits it (SplitPlan, rows_plan), its rows are summed in row order and its splits folded in split
// order by the code the single kernels run (psf_focus_sum_chunk, focus_sums_item, focus_spread_item, geo_otf_item, otf_rows_thread,
// otf_cols_thread), and a plane's value does not depend on the chunk that ran it: block c equals the single call on configuration c's rows
// bit for bit.  A configuration without rows has no work item; what it reads is filled on the host as the single call fills it.

// What the four entries end their checks on: the ranges of the slot's rows over the configurations (H = 0: every count is 0, no device is
// touched) and the rows themselves.
static int sweep_focus_rows(const char* who, bmo_trace_result* res, int32_t detector, int32_t n_configs, Ranges& R, const double*& hits, int64_t& H) {
    H = res->det_count[detector];
    hits = nullptr;
    if (H > 0) return resident_rows(who, res, detector, H, n_configs, R, hits);
    R.begin.assign((size_t)n_configs, 0);
    R.count.assign((size_t)n_configs, 0);
    return BMO_OK;
}

// frames [K] from poses and axes [K][3]
static std::vector<FocusFrame> focus_frames(size_t K, const double* origins, const double* e1s, const double* e2s, const double* axes) {
    std::vector<FocusFrame> F(K);
    for (size_t c = 0; c < K; ++c) F[c] = focus_frame(origins + 3 * c, e1s + 3 * c, e2s + 3 * c, axes + 3 * c);
    return F;
}

extern "C" int bmo_psf_focus_stats_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                         const double* axes, const double* offsets, int32_t n_planes, double* stats, double* kernel_ms) {
    const char* who = "bmo_psf_focus_stats_sweep";
    if (!res || !origins || !e1s || !e2s || !axes || !offsets || !stats || n_planes <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_focus_stats_sweep: bad argument (null pointer, n_planes <= 0)");
    if (int rc = slot_check(who, res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    const unsigned chunks = (unsigned)((n_planes + FOCUS_STAT_MP - 1) / FOCUS_STAT_MP);
    if (chunks > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more planes than one launch holds");
    if (kernel_ms) *kernel_ms = 0.0;
    Ranges R;
    const double* hits;
    int64_t H;
    if (int rc = sweep_focus_rows(who, res, detector, n_configs, R, hits, H)) return rc;
    const size_t K = (size_t)n_configs, M = (size_t)n_planes;
    if (H > 0) {
        RowPasses P(R);
        if (int rc = P.items(who)) return rc;
        // the records are [configuration][plane][split]: to the reduces a (configuration, plane) pair is a range of the configuration's splits
        P.ranges.resize(K * M);
        for (size_t c = 0; c < K; ++c)
            for (size_t m = 0; m < M; ++m) {
                const SplitCfg& C = P.plan.cfg[c];
                P.ranges[c * M + m] = SplitCfg{(int64_t)M * C.first_work + (int64_t)m * C.n_splits, C.n_splits, 0};
            }
        const size_t o_cfg = P.up.add(P.plan.cfg), o_frames = P.up.add(focus_frames(K, origins, e1s, e2s, axes)), o_off = P.up.add(offsets, K * M),
                     o_count = P.up.add(R.count);
        DevBuf d_stats, d_mid;
        int rc;
        if ((rc = d_stats.alloc(K * M * BMO_FOCUS_STAT_N * 8)) || (rc = d_mid.alloc(K * M * sizeof(double2))) || (rc = P.begin<FocusSumA, FocusSumC>())) return rc;
        P.grid.y = chunks;  // a workgroup per work item and chunk of planes
        const SplitCfg* d_cfg = P.up.at<SplitCfg>(o_cfg);
        const FocusFrame* d_frames = P.up.at<FocusFrame>(o_frames);
        const double* d_off = P.up.at<double>(o_off);
        double* const g_stats = (double*)d_stats.p;
        double2* const g_mid = (double2*)d_mid.p;
        P.pass<FocusSumA>(psf_focus_sums_list_kernel, FocusSumsListFinish{P.up.at<int64_t>(o_count), n_planes, g_stats, g_mid}, hits, P.work(), d_cfg, d_frames, d_off,
                          n_planes);
        P.pass<FocusSumC>(psf_focus_spread_list_kernel, FocusSpreadFinish{g_stats}, hits, P.work(), d_cfg, d_frames, d_off, n_planes, (const double2*)g_mid);
        if ((rc = P.end(kernel_ms))) return rc;
        HIP_TRY(hipMemcpy(stats, g_stats, K * M * BMO_FOCUS_STAT_N * 8, hipMemcpyDeviceToHost));
    }
    for (size_t c = 0; c < K; ++c)
        if (R.count[c] == 0) fill_empty_stats(stats + c * M * BMO_FOCUS_STAT_N, M, BMO_FOCUS_STAT_N);
    return BMO_OK;
}

// The stacks of the K = R.count.size() configurations from the device rows `hits` (some configuration has rows), left on the device: d_int
// [K][n_planes][n * n], and d_field likewise when want_field; a configuration without rows reads zeros.  poses [K][3], disp
// [K][n_planes][3], axes [K][n].  `timer` runs from the first launch; the caller may queue more behind the stacks on stream 0 and stop it again.
static int psf_focus_stack_sweep(const double* hits, const Ranges& R, const double* origins, const double* e1s, const double* e2s, const double* disp, int32_t n_planes,
                                 const double* xs, const double* zs, int32_t n, bool want_field, DevBuf& d_int, DevBuf& d_field, EventTimer& timer, double* kernel_ms) {
    const size_t K = R.count.size();
    const int64_t n_pts = (int64_t)n * n;
    const unsigned pt_blocks = (unsigned)((n_pts + 255) / 256);
    const size_t n_out = K * (size_t)n_planes * (size_t)n_pts;
    hipStream_t st = 0;
    // planes per pass: whole chunks, partial sums of at most 1 GiB for the configuration of most splits (one chunk if a single one needs
    // more); the launches: SplitPlan's rule on the pass_planes * n_pts partial sums an item writes
    int64_t most = 1;
    for (int64_t n_hits : R.count) {
        int64_t n_splits, hits_per_split;
        psf_splits(n_hits, pt_blocks, n_splits, hits_per_split);
        most = std::max(most, n_splits);
    }
    const int64_t fit = ((int64_t)1 << 30) / (most * n_pts * (int64_t)sizeof(double2)) / PSF_FOCUS_MP * PSF_FOCUS_MP;
    const int32_t per_pass = (int32_t)std::min<int64_t>({std::max<int64_t>(fit, PSF_FOCUS_MP), (int64_t)65535 * PSF_FOCUS_MP, (int64_t)n_planes});
    const SplitPlan plan(R, pt_blocks, (int64_t)per_pass * n_pts, psf_splits);  // bmo_psf_intensity's splits of every configuration's rows on this grid
    Packed up;
    const size_t o_cfg = up.add(plan.cfg), o_work = up.add(plan.work), o_pose = up.add(psf_poses(K, origins, e1s, e2s)), o_xs = up.add(xs, K * (size_t)n),
                 o_zs = up.add(zs, K * (size_t)n), o_d = up.add(disp, K * (size_t)n_planes * 3);
    int rc;
    if ((rc = up.upload(st)) || (rc = d_int.alloc(n_out * sizeof(double))) || (want_field && (rc = d_field.alloc(n_out * sizeof(double2))))) return rc;
    for (int32_t m_pass = 0; m_pass < n_planes; m_pass += per_pass) {
        const int32_t pass_planes = std::min(per_pass, n_planes - m_pass);
        auto accumulate = [&](dim3, const SplitPlan::Launch& L, double2* partial) {
            auto launch = [&](auto mp, int32_t m_first, int32_t chunks) {
                hipLaunchKernelGGL(psf_focus_accumulate_list_kernel<decltype(mp)::value>, dim3(pt_blocks, (unsigned)L.nw, (unsigned)chunks), dim3(256), 0, st, hits,
                                   up.at<SplitWork>(o_work), L.w0, up.at<PsfPose>(o_pose), up.at<double>(o_xs), up.at<double>(o_zs), n, up.at<double>(o_d), n_planes,
                                   m_first, m_pass, pass_planes, partial);
            };
            const int32_t full = pass_planes / PSF_FOCUS_MP, rest = pass_planes % PSF_FOCUS_MP, m_rest = m_pass + full * PSF_FOCUS_MP;
            if (full > 0) launch(std::integral_constant<int, PSF_FOCUS_MP>{}, m_pass, full);
            if (rest > 8) launch(std::integral_constant<int, 16>{}, m_rest, 1);  // the slots past the last plane run idle
            else if (rest > 4) launch(std::integral_constant<int, 8>{}, m_rest, 1);
            else if (rest > 2) launch(std::integral_constant<int, 4>{}, m_rest, 1);
            else if (rest > 1) launch(std::integral_constant<int, 2>{}, m_rest, 1);
            else if (rest > 0) launch(std::integral_constant<int, 1>{}, m_rest, 1);
        };
        const int64_t pass_pts = (int64_t)pass_planes * n_pts;
        const PsfStackFinish finish{(double*)d_int.p + (int64_t)m_pass * n_pts, want_field ? (double2*)d_field.p + (int64_t)m_pass * n_pts : nullptr, pass_pts,
                                    (int64_t)n_planes * n_pts};
        if ((rc = split_reduce(plan, up.at<SplitCfg>(o_cfg), pass_pts, st, timer, kernel_ms, accumulate, finish))) return rc;
    }
    return BMO_OK;
}

extern "C" int bmo_psf_through_focus_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                           const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, double* out_intensity,
                                           double* out_field, double* kernel_ms) {
    const char* who = "bmo_psf_through_focus_sweep";
    if (!res || !origins || !e1s || !e2s || !displacements || !xs || !zs || !out_intensity || n <= 0 || n_planes <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_through_focus_sweep: bad argument (null pointer, n <= 0, n_planes <= 0)");
    if (int rc = slot_check(who, res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    if (kernel_ms) *kernel_ms = 0.0;
    Ranges R;
    const double* hits;
    int64_t H;
    if (int rc = sweep_focus_rows(who, res, detector, n_configs, R, hits, H)) return rc;
    const size_t n_out = (size_t)n_configs * (size_t)n_planes * (size_t)n * (size_t)n;
    if (H == 0) {  // every configuration reads like a call with n_hits = 0
        std::fill(out_intensity, out_intensity + n_out, 0.0);
        if (out_field) std::fill(out_field, out_field + 2 * n_out, 0.0);
        return BMO_OK;
    }
    DevBuf d_int, d_field;
    EventTimer timer;
    if (int rc = psf_focus_stack_sweep(hits, R, origins, e1s, e2s, displacements, n_planes, xs, zs, n, out_field != nullptr, d_int, d_field, timer, kernel_ms)) return rc;
    HIP_TRY(hipMemcpy(out_intensity, d_int.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    if (out_field) HIP_TRY(hipMemcpy(out_field, d_field.p, n_out * sizeof(double2), hipMemcpyDeviceToHost));
    return BMO_OK;
}

// block c of the transfer functions of a sweep as a configuration without rows reads it
static void otf_fill_empty_configs(const Ranges& R, size_t n_planes, size_t n_freqs, double* otf, double* mtf, double* sums) {
    const size_t n_pairs = n_planes * n_freqs;
    for (size_t c = 0; c < R.count.size(); ++c)
        if (R.count[c] == 0) otf_fill_empty(n_pairs, n_planes, otf + 2 * c * n_pairs, mtf + c * n_pairs, sums + c * n_planes);
}

extern "C" int bmo_psf_geo_otf_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                     const double* axes, const double* offsets, const double* centers, int32_t n_planes, const double* freqs, int32_t n_freqs,
                                     double* otf, double* mtf, double* sums, double* kernel_ms) {
    const char* who = "bmo_psf_geo_otf_sweep";
    if (!res || !origins || !e1s || !e2s || !axes || !offsets || !freqs || !otf || !mtf || !sums || n_planes <= 0 || n_freqs <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_geo_otf_sweep: bad argument (null pointer, n_planes <= 0, n_freqs <= 0)");
    if (!otf_freqs_ok(freqs, n_freqs)) return fail(BMO_ERR_INVALID, "bmo_psf_geo_otf_sweep: a frequency is not finite");
    if (int rc = slot_check(who, res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    int mp = 1;
    while (mp < GEO_OTF_MP && mp < n_planes) mp *= 2;
    const unsigned chunks = (unsigned)((n_planes + mp - 1) / mp), f_blocks = (unsigned)(((int64_t)n_freqs + 256 / mp - 1) / (256 / mp));
    if (chunks > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more planes than one launch holds");
    if (kernel_ms) *kernel_ms = 0.0;
    Ranges R;
    const double* hits;
    int64_t H;
    if (int rc = sweep_focus_rows(who, res, detector, n_configs, R, hits, H)) return rc;
    const size_t K = (size_t)n_configs;
    const int64_t n_pairs = (int64_t)n_planes * n_freqs;
    if (H > 0) {
        // the splits of the statistics passes (S is one of their sums), in launches of consecutive configurations by SplitPlan's rule
        const SplitPlan plan = rows_plan(R, n_pairs);
        unsigned n_items = 0;
        if (int rc = rows_items(plan, who, n_items)) return rc;
        // a pair's value does not depend on the pairs asked for along with it: a caller with more of them splits the call
        if (plan.max_nw * n_pairs > ((int64_t)1 << 32) / (int64_t)sizeof(double2))
            return fail(BMO_ERR_LIMIT, std::string(who) + ": the partial sums of n_planes * n_freqs pairs pass 4 GiB; ask for them in several calls");
        hipStream_t st = 0;
        Packed up;
        const size_t o_cfg = up.add(plan.cfg), o_work = up.add(plan.work), o_frames = up.add(focus_frames(K, origins, e1s, e2s, axes)),
                     o_off = up.add(offsets, K * (size_t)n_planes), o_freq = up.add(freqs, (size_t)n_freqs * 2);
        const size_t o_cen = centers ? up.add(centers, K * (size_t)n_planes * 2) : 0;
        DevBuf d_partial, d_records, d_s, d_otf, d_mtf, d_sums;
        int rc;
        if ((rc = up.upload(st)) || (rc = d_partial.alloc((size_t)plan.max_nw * (size_t)n_pairs * sizeof(double2))) ||
            (rc = d_records.alloc((size_t)n_items * sizeof(GeoOtfSum))) || (rc = d_s.alloc(K * 8)) || (rc = d_otf.alloc(K * (size_t)n_pairs * sizeof(double2))) ||
            (rc = d_mtf.alloc(K * (size_t)n_pairs * 8)) || (rc = d_sums.alloc(K * (size_t)n_planes * 8)))
            return rc;
        const SplitCfg* d_cfg = up.at<SplitCfg>(o_cfg);
        const double2* d_cen = centers ? up.at<double2>(o_cen) : nullptr;
        EventTimer timer;
        if ((rc = timer.start(st))) return rc;
        for (const SplitPlan::Launch& L : plan.launches) {
            auto launch = [&](auto MP) {
                hipLaunchKernelGGL(psf_geo_otf_list_kernel<decltype(MP)::value>, dim3(f_blocks, (unsigned)L.nw, chunks), dim3(256), 0, st, hits, up.at<SplitWork>(o_work),
                                   L.w0, up.at<FocusFrame>(o_frames), up.at<double>(o_off), d_cen, n_planes, up.at<double2>(o_freq), n_freqs, (double2*)d_partial.p,
                                   (GeoOtfSum*)d_records.p);
            };
            if (L.nw > 0) {
                if (mp == 1) launch(std::integral_constant<int, 1>{});
                else if (mp == 2) launch(std::integral_constant<int, 2>{});
                else if (mp == 4) launch(std::integral_constant<int, 4>{});
                else launch(std::integral_constant<int, GEO_OTF_MP>{});
            }
            sum_reduce<GeoOtfSum>((unsigned)L.nc, st, d_cfg + L.c0, d_records, GeoOtfSumListFinish{(double*)d_s.p + L.c0});
            hipLaunchKernelGGL(psf_geo_otf_reduce_list_kernel, dim3((unsigned)((n_pairs + 255) / 256), (unsigned)L.nc), dim3(256), 0, st, d_cfg, L.c0, L.w0,
                               (const double2*)d_partial.p, n_pairs, n_freqs, (const double*)d_s.p, (double2*)d_otf.p, (double*)d_mtf.p, (double*)d_sums.p);
        }
        if ((rc = timer.stop(kernel_ms))) return rc;
        HIP_TRY(hipMemcpy(otf, d_otf.p, K * (size_t)n_pairs * sizeof(double2), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(mtf, d_mtf.p, K * (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sums, d_sums.p, K * (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    }
    otf_fill_empty_configs(R, (size_t)n_planes, (size_t)n_freqs, otf, mtf, sums);
    return BMO_OK;
}

extern "C" int bmo_psf_otf_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* origins, const double* e1s, const double* e2s,
                                 const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* freqs, int32_t n_freqs,
                                 double* otf, double* mtf, double* sums, double* out_intensity, double* kernel_ms) {
    const char* who = "bmo_psf_otf_sweep";
    if (!res || !origins || !e1s || !e2s || !displacements || !xs || !zs || !freqs || !otf || !mtf || !sums || n <= 0 || n_planes <= 0 || n_freqs <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_otf_sweep: bad argument (null pointer, n <= 0, n_planes <= 0, n_freqs <= 0)");
    if (!otf_freqs_ok(freqs, n_freqs)) return fail(BMO_ERR_INVALID, "bmo_psf_otf_sweep: a frequency is not finite");
    if (int rc = slot_check(who, res, detector, BMO_OBJ_PSFDETECTOR, true, n_configs)) return rc;
    const size_t K = (size_t)n_configs;
    const int64_t n_images = (int64_t)n_configs * n_planes, n_pairs = n_images * n_freqs, n_rowsums = n_images * (n_freqs + 1) * n;
    if ((n_rowsums + 255) / 256 > (int64_t)0x7fffffff) return fail(BMO_ERR_LIMIT, std::string(who) + ": more row sums than one launch holds");
    if (kernel_ms) *kernel_ms = 0.0;
    Ranges R;
    const double* hits;
    int64_t H;
    if (int rc = sweep_focus_rows(who, res, detector, n_configs, R, hits, H)) return rc;
    const size_t n_out = (size_t)n_images * (size_t)n * (size_t)n;
    if (H > 0) {
        hipStream_t st = 0;
        DevBuf d_int, d_field, d_rowsum, d_otf, d_mtf, d_sums;
        Packed up;
        const size_t o_xs = up.add(xs, K * (size_t)n), o_zs = up.add(zs, K * (size_t)n), o_freq = up.add(freqs, (size_t)n_freqs * 2);
        int rc;
        if ((rc = up.upload(st)) || (rc = d_rowsum.alloc((size_t)n_rowsums * sizeof(double2))) || (rc = d_otf.alloc((size_t)n_pairs * sizeof(double2))) ||
            (rc = d_mtf.alloc((size_t)n_pairs * 8)) || (rc = d_sums.alloc((size_t)n_images * 8)))
            return rc;
        EventTimer timer;
        if ((rc = psf_focus_stack_sweep(hits, R, origins, e1s, e2s, displacements, n_planes, xs, zs, n, false, d_int, d_field, timer, kernel_ms))) return rc;
        hipLaunchKernelGGL(psf_otf_rows_list_kernel, dim3((unsigned)((n_rowsums + 255) / 256)), dim3(256), 0, st, (const double*)d_int.p, up.at<double>(o_xs), n_planes, n,
                           up.at<double2>(o_freq), n_freqs, n_rowsums, (double2*)d_rowsum.p);
        hipLaunchKernelGGL(psf_otf_cols_list_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, (const double2*)d_rowsum.p, up.at<double>(o_zs), n_planes, n,
                           up.at<double2>(o_freq), n_freqs, n_pairs, (double2*)d_otf.p, (double*)d_mtf.p, (double*)d_sums.p);
        if ((rc = timer.stop(kernel_ms))) return rc;
        HIP_TRY(hipMemcpy(otf, d_otf.p, (size_t)n_pairs * sizeof(double2), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(mtf, d_mtf.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_images * 8, hipMemcpyDeviceToHost));
        if (out_intensity) HIP_TRY(hipMemcpy(out_intensity, d_int.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    } else if (out_intensity) {
        std::fill(out_intensity, out_intensity + n_out, 0.0);
    }
    // a configuration without rows: its images are zeros already; its transfer function must not depend on its axes (NaN where the caller
    // has no window for it)
    otf_fill_empty_configs(R, (size_t)n_planes, (size_t)n_freqs, otf, mtf, sums);
    return BMO_OK;
}

// ====================================================================================================================
// Encircled-energy read-out (include/bmo.h "Encircled-energy read-out"): the share of the light inside a circle or a square of half-size R
// about a centre, for a list of R.  A point has one key: r2 = ax * ax + az * az (circle) or max(|ax|, |az|) (square), and it is inside
// radius k iff key <= thr_k, thr_k = R_k * R_k or R_k, computed once on the host.  A NaN key compares false: outside every radius.
//
// Geometric (bmo_psf_geo_ee).  psf_geo_otf_kernel's shape with a (plane, radius) pair for a (plane, frequency) pair: a workgroup owns one
// split of the rows (spot_splits), one chunk of MP planes and 256 / MP radii; per staged tile lane r propagates row r to the chunk's planes
// and writes ONE double per (plane, row), its key, to LDS laid out [plane][row]; every lane then walks the tile with broadcast reads, a
// compare, a masked add of proj and a masked count: no division, root or transcendental inside the walk.  18 KB of row tile + MP * 2 KB:
// 34 KB at MP = 8, four workgroups per CU.  A pair's sum runs over the rows of a split in row order (a row outside adds +0.0 to a sum
// that started at +0.0: the same number as adding nothing), the splits are folded in split order.  S is GeoOtfSum's, summed as the focus
// statistics sum it.
//
// Diffraction (bmo_psf_ee).  psf_focus_stack's images summed where they lie, in the row / column shape of psf_otf_rows_kernel /
// psf_otf_cols_kernel, twice: the moments (S and the centroid), then the energies about the centre.
//
// Spot (bmo_spot_ee, bmo_spot_ee_sweep).  spot_image_kernel's shape with a radial key for a bin: the thresholds sorted on the host, a
// row's bin the number of thresholds below its key (a binary search; K for a NaN), counted into a per-workgroup LDS histogram of K + 1
// bins by spot_add and added to the configuration's with 64-bit atomics; a cumulative pass per configuration turns bins into counts (a
// row is inside sorted radius s iff its bin is <= s) and writes them in the caller's order.
namespace {

constexpr int GEO_EE_MP = 8;  // planes per chunk of a stack; a stack of fewer planes runs the next power of two

struct EePartial {
    double e;
    long long n;
};
static_assert(sizeof(EePartial) == 16, "16 bytes per split, plane and radius");

// the key of a point at (ax, az) from the centre.  The square's is the larger of |ax| and |az| and NaN if either is
__device__ __forceinline__ double ee_key(double ax, double az, int32_t shape) {
    if (shape == 0) return ax * ax + az * az;
    const double fx = fabs(ax), fz = fabs(az);
    return (fx >= fz || fx != fx) ? fx : fz;
}

// split blockIdx.y (work item) of the rows, planes blockIdx.z * MP .., radii blockIdx.x * (256 / MP) ..; partial: [item][plane][radius]
template <int MP>
__global__ __launch_bounds__(256) void psf_geo_ee_kernel(const double* __restrict__ hits, const SplitWork* __restrict__ work, FocusFrame F,
                                                         const double* __restrict__ offsets, const double2* __restrict__ centers, int32_t n_planes,
                                                         int32_t shape, const double* __restrict__ thr, int32_t n_radii, EePartial* __restrict__ partial,
                                                         GeoOtfSum* __restrict__ sums) {
    constexpr int RB = 256 / MP;
    static_assert(MP >= 1 && MP <= 8 && 256 % MP == 0, "a chunk of planes divides the workgroup");
    __shared__ double tile[PSF_TILE * 9];
    __shared__ double key[MP * PSF_TILE];
    const SplitWork W = work[blockIdx.y];
    const int32_t m0 = (int32_t)blockIdx.z * MP;
    const int mcnt = n_planes - m0 < MP ? n_planes - m0 : MP;  // planes of this chunk; the slots past them repeat its first and are not stored
    d3 o[MP];
    double2 c[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int32_t mm = m0 + (m < mcnt ? m : 0);
        o[m] = focus_origin(F, offsets[mm]);
        c[m] = centers ? centers[mm] : make_double2(0.0, 0.0);
    }
    const int ml = (int)threadIdx.x / RB;
    const int32_t k = (int32_t)blockIdx.x * RB + (int)threadIdx.x % RB;
    const bool live = ml < mcnt && k < n_radii;
    const double t = live ? thr[k] : 0.0;
    GeoOtfSum a = sum_identity<GeoOtfSum>();
    double e = 0.0;
    long long n = 0;
    for (int64_t base = W.h0; base < W.h1; base += PSF_TILE) {
        const int cnt = (int)(W.h1 - base < PSF_TILE ? W.h1 - base : PSF_TILE);
        psf_stage_rows(hits, base, cnt, tile);  // its first sync: the walk over the tile before is done
        if ((int)threadIdx.x < cnt) {
            const double* r = tile + 9 * threadIdx.x;
            const double den = focus_den(r, F);
            a.s += r[7];
            a.bad += den == 0.0 ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < MP; ++m) {
                double x, z;
                focus_local(r, F, o[m], den, x, z);
                key[m * PSF_TILE + threadIdx.x] = ee_key(x - c[m].x, z - c[m].y, shape);
            }
        }
        __syncthreads();
        if (live) {
            const double* p = key + ml * PSF_TILE;
            for (int h = 0; h < cnt; ++h) {
                const bool in = p[h] <= t;
                e += in ? tile[9 * h + 7] : 0.0;
                n += in ? 1 : 0;
            }
        }
    }
    if (live) partial[((int64_t)blockIdx.y * n_planes + (m0 + ml)) * n_radii + k] = EePartial{e, n};
    if (blockIdx.x == 0 && blockIdx.z == 0) {  // uniform over the workgroup: one record per work item
        a = sum_wg_reduce(a);
        if (threadIdx.x == 0) sums[blockIdx.y] = a;
    }
}

// pair (plane, radius) = blockIdx.x * 256 + threadIdx.x: its partial sums folded in split order; energy, ee, count (optional) and, from
// the pairs of radius 0, sums
__global__ void psf_geo_ee_reduce_kernel(const EePartial* __restrict__ partial, int32_t n_splits, int64_t n_pairs, int32_t n_radii, const double* __restrict__ s_all,
                                         double* __restrict__ ee, double* __restrict__ energy, long long* __restrict__ count, double* __restrict__ sums) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    double e = 0.0;
    long long n = 0;
    for (int32_t s = 0; s < n_splits; ++s) {
        const EePartial v = partial[(int64_t)s * n_pairs + q];
        e += v.e;
        n += v.n;
    }
    const double S = *s_all;
    if (S != S) e = knan();  // a row parallel to the planes (or a NaN proj): no energy
    energy[q] = e;
    ee[q] = e / S;
    if (count) count[q] = n;
    if (q % n_radii == 0) sums[q / n_radii] = S;
}

// Diffraction, the moments: thread (plane m, row j) sums image row j and its first x moment, i ascending
__global__ void psf_ee_moment_rows_kernel(const double* __restrict__ img, const double* __restrict__ xs, int32_t n, int64_t n_threads, double2* __restrict__ rowmom) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;  // n_planes * n
    const double* row = img + t * n;
    double s = 0.0, sx = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        s += row[i];
        sx += row[i] * xs[i];
    }
    rowmom[t] = make_double2(s, sx);  // [m][j]
}

// thread (plane m): the row moments summed, j ascending; sums and the centre used (the given one, or the intensity centroid)
__global__ void psf_ee_moment_cols_kernel(const double2* __restrict__ rowmom, const double* __restrict__ zs, int32_t n, int32_t n_planes,
                                          const double2* __restrict__ centers, double* __restrict__ sums, double2* __restrict__ centers_out) {
    const int32_t m = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (m >= n_planes) return;
    const double2* r = rowmom + (int64_t)m * n;
    double S = 0.0, sx = 0.0, sz = 0.0;
    for (int32_t j = 0; j < n; ++j) {
        S += r[j].x;
        sx += r[j].y;
        sz += r[j].x * zs[j];
    }
    sums[m] = S;
    centers_out[m] = centers ? centers[m] : make_double2(sx / S, sz / S);
}

// thread (plane m, radius k, row j): the samples of image row j inside radius k about the plane's centre, i ascending
__global__ void psf_ee_rows_kernel(const double* __restrict__ img, const double* __restrict__ xs, const double* __restrict__ zs, int32_t n,
                                   const double2* __restrict__ cen, int32_t shape, const double* __restrict__ thr, int32_t n_radii, int64_t n_threads,
                                   double* __restrict__ rowsum) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_threads) return;  // n_planes * n_radii * n
    const int32_t j = (int32_t)(t % n), k = (int32_t)(t / n % n_radii);
    const int64_t m = t / n / n_radii;
    const double* row = img + (m * n + j) * n;
    const double2 c = cen[m];
    const double az = zs[j] - c.y, th = thr[k];
    double e = 0.0;
    for (int32_t i = 0; i < n; ++i) e += ee_key(xs[i] - c.x, az, shape) <= th ? row[i] : 0.0;
    rowsum[t] = e;  // [m][k][j]
}

// thread (plane m, radius k): the row sums added, j ascending
__global__ void psf_ee_cols_kernel(const double* __restrict__ rowsum, int32_t n, int32_t n_radii, int64_t n_pairs, const double* __restrict__ sums,
                                   double* __restrict__ ee, double* __restrict__ energy) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const double* r = rowsum + q * n;
    double e = 0.0;
    for (int32_t j = 0; j < n; ++j) e += r[j];
    energy[q] = e;
    ee[q] = e / sums[q / n_radii];
}

constexpr int SPOT_EE_MAX_RADII = 4096;

// work item blockIdx.x: the bins of its rows (the number of sorted thresholds below the row's key; n_radii for a NaN) added to hist[cfg],
// [n_radii + 1] each.  LDS: the thresholds, then the counters.
__global__ __launch_bounds__(256) void spot_ee_kernel(const double* __restrict__ rows, int32_t cols, const SplitWork* __restrict__ work,
                                                      const double2* __restrict__ centers, int32_t shape, const double* __restrict__ thr, int32_t n_radii,
                                                      unsigned long long* __restrict__ hist) {
    __shared__ double sh_thr[SPOT_EE_MAX_RADII];
    __shared__ uint32_t sh_hist[SPOT_EE_MAX_RADII + 1];
    const SplitWork W = work[blockIdx.x];
    const double2 c = centers[W.cfg];
    for (int32_t b = threadIdx.x; b < n_radii; b += 256) sh_thr[b] = thr[b];
    for (int32_t b = threadIdx.x; b <= n_radii; b += 256) sh_hist[b] = 0;
    __syncthreads();
    for (int64_t base = W.h0; base < W.h1; base += 256) {  // workgroup-uniform trips: spot_add needs whole waves
        const int64_t h = base + threadIdx.x;
        const bool live = h < W.h1;
        int32_t bin = n_radii;
        if (live) {
            const double* r = rows + h * cols;
            const double v = ee_key(r[0] - c.x, r[1] - c.y, shape);
            if (v == v) {
                int32_t lo = 0, hi = n_radii;  // the first threshold that is not below v
                while (lo < hi) {
                    const int32_t mid = (lo + hi) >> 1;
                    if (sh_thr[mid] < v) lo = mid + 1;
                    else hi = mid;
                }
                bin = lo;
            }
        }
        spot_add(sh_hist, bin, live);
    }
    __syncthreads();
    unsigned long long* out = hist + (int64_t)W.cfg * (n_radii + 1);
    for (int32_t b = threadIdx.x; b <= n_radii; b += 256) {
        const uint32_t v = sh_hist[b];
        if (v) atomicAdd(&out[b], (unsigned long long)v);
    }
}

// configuration blockIdx.x: inside[cfg][perm[s]] = hist[cfg][0] + .. + hist[cfg][s].  Lane l sums bins l * per .. in order, a scan over the
// lanes' totals gives each its start.
__global__ __launch_bounds__(256) void spot_ee_cumulate_kernel(const unsigned long long* __restrict__ hist, const int32_t* __restrict__ perm, int32_t n_radii,
                                                               long long* __restrict__ inside) {
    __shared__ unsigned long long tot[256];
    const unsigned long long* h = hist + (int64_t)blockIdx.x * (n_radii + 1);
    long long* out = inside + (int64_t)blockIdx.x * n_radii;
    const int32_t per = (n_radii + 255) / 256, b0 = (int32_t)threadIdx.x * per, b1 = b0 + per < n_radii ? b0 + per : n_radii;
    unsigned long long s = 0;
    for (int32_t b = b0; b < b1; ++b) s += h[b];
    tot[threadIdx.x] = s;
    __syncthreads();
    unsigned long long run = 0;
    for (int l = 0; l < (int)threadIdx.x; ++l) run += tot[l];
    for (int32_t b = b0; b < b1; ++b) {
        run += h[b];
        out[perm[b]] = (long long)run;
    }
}

}  // namespace

// what the encircled-energy entries refuse of their shape, radii and centres; thr: the thresholds the kernels compare with
static bool ee_args_ok(int32_t shape, const double* radii, int32_t n_radii, const double* centers, int64_t n_centers, std::vector<double>& thr) {
    if (shape < 0 || shape > 1) return false;
    thr.resize((size_t)n_radii);
    for (int32_t k = 0; k < n_radii; ++k) {
        if (!std::isfinite(radii[k]) || radii[k] < 0) return false;
        thr[(size_t)k] = shape == 0 ? radii[k] * radii[k] : radii[k];
    }
    for (int64_t q = 0; centers && q < 2 * n_centers; ++q)
        if (!std::isfinite(centers[q])) return false;
    return true;
}

// The geometric encircled energy of the n_hits > 0 device rows `hits` [..][9].
static int psf_geo_ee_read(const double* hits, int64_t n_hits, const double* origin, const double* e1, const double* e2, const double* axis, const double* offsets,
                           const double* centers, int32_t n_planes, int32_t shape, const std::vector<double>& thr, double* ee, double* energy, int64_t* count,
                           double* sums, double* kernel_ms, const char* who) {
    const int32_t n_radii = (int32_t)thr.size();
    RowPasses P(Ranges{{0}, {n_hits}});  // the plan, the upload and the reduce of the statistics passes: S is one
    if (int rc = P.items(who)) return rc;
    const FocusFrame F = focus_frame(origin, e1, e2, axis);
    int mp = 1;
    while (mp < GEO_EE_MP && mp < n_planes) mp *= 2;
    const unsigned chunks = (unsigned)((n_planes + mp - 1) / mp), r_blocks = (unsigned)(((int64_t)n_radii + 256 / mp - 1) / (256 / mp));
    const int64_t n_pairs = (int64_t)n_planes * n_radii;
    if (chunks > 65535 || P.n_items > 65535) return fail(BMO_ERR_LIMIT, std::string(who) + ": more planes than one launch holds");
    // a pair's value does not depend on the pairs asked for along with it: a caller with more of them splits the call
    if ((int64_t)P.n_items * n_pairs > ((int64_t)1 << 32) / (int64_t)sizeof(EePartial))
        return fail(BMO_ERR_LIMIT, std::string(who) + ": the partial sums of n_planes * n_radii pairs pass 4 GiB; ask for them in several calls");
    const size_t o_off = P.up.add(offsets, (size_t)n_planes), o_thr = P.up.add(thr);
    const size_t o_cen = centers ? P.up.add(centers, (size_t)n_planes * 2) : 0;
    DevBuf d_partial, d_s, d_ee, d_energy, d_count, d_sums;
    int rc;
    if ((rc = d_partial.alloc((size_t)P.n_items * (size_t)n_pairs * sizeof(EePartial))) || (rc = d_s.alloc(8)) || (rc = d_ee.alloc((size_t)n_pairs * 8)) ||
        (rc = d_energy.alloc((size_t)n_pairs * 8)) || (count && (rc = d_count.alloc((size_t)n_pairs * 8))) || (rc = d_sums.alloc((size_t)n_planes * 8)) ||
        (rc = P.begin<GeoOtfSum>()))
        return rc;
    const double2* d_cen = centers ? P.up.at<double2>(o_cen) : nullptr;
    auto launch = [&](auto MP) {
        hipLaunchKernelGGL(psf_geo_ee_kernel<decltype(MP)::value>, dim3(r_blocks, P.n_items, chunks), dim3(256), 0, P.st, hits, P.work(), F, P.up.at<double>(o_off), d_cen,
                           n_planes, shape, P.up.at<double>(o_thr), n_radii, (EePartial*)d_partial.p, (GeoOtfSum*)P.records.p);
    };
    if (mp == 1) launch(std::integral_constant<int, 1>{});
    else if (mp == 2) launch(std::integral_constant<int, 2>{});
    else if (mp == 4) launch(std::integral_constant<int, 4>{});
    else launch(std::integral_constant<int, GEO_EE_MP>{});
    sum_reduce<GeoOtfSum>(1u, P.st, P.cfg(), P.records, GeoOtfSumFinish{(double*)d_s.p});
    hipLaunchKernelGGL(psf_geo_ee_reduce_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, P.st, (const EePartial*)d_partial.p, (int32_t)P.n_items, n_pairs,
                       n_radii, (const double*)d_s.p, (double*)d_ee.p, (double*)d_energy.p, count ? (long long*)d_count.p : nullptr, (double*)d_sums.p);
    if ((rc = P.end(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(ee, d_ee.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(energy, d_energy.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    if (count) HIP_TRY(hipMemcpy(count, d_count.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_geo_ee(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                              const double axis[3], const double* offsets, const double* centers, int32_t n_planes, int32_t shape, const double* radii, int32_t n_radii,
                              int32_t device, double* ee, double* energy, int64_t* count, double* sums, double* kernel_ms) {
    if (!origin || !e1 || !e2 || !axis || !offsets || !radii || !ee || !energy || !sums || n_planes <= 0 || n_radii <= 0 || n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_geo_ee: bad argument (null pointer, n_planes <= 0, n_radii <= 0, n_hits < 0)");
    std::vector<double> thr;
    if (!ee_args_ok(shape, radii, n_radii, centers, n_planes, thr))
        return fail(BMO_ERR_INVALID, "bmo_psf_geo_ee: shape must be 0 or 1, every radius finite and >= 0, every centre finite");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_geo_ee", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    if (n_hits == 0) {
        const size_t n_pairs = (size_t)n_planes * (size_t)n_radii;
        std::fill(ee, ee + n_pairs, std::nan(""));
        std::fill(energy, energy + n_pairs, 0.0);
        if (count) std::fill(count, count + n_pairs, (int64_t)0);
        std::fill(sums, sums + n_planes, 0.0);
        return BMO_OK;
    }
    return psf_geo_ee_read(hits, n_hits, origin, e1, e2, axis, offsets, centers, n_planes, shape, thr, ee, energy, count, sums, kernel_ms, "bmo_psf_geo_ee");
}

extern "C" int bmo_psf_ee(const double* hits, int64_t n_hits, int32_t hits_on_device, const double origin[3], const double e1[3], const double e2[3],
                          const double* displacements, int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* centers, int32_t shape,
                          const double* radii, int32_t n_radii, int32_t device, double* ee, double* energy, double* sums, double* centers_out, double* out_intensity,
                          double* kernel_ms) {
    if (!origin || !e1 || !e2 || !displacements || !xs || !zs || !radii || !ee || !energy || !sums || !centers_out || n <= 0 || n_planes <= 0 || n_radii <= 0 ||
        n_hits < 0 || (n_hits > 0 && !hits))
        return fail(BMO_ERR_INVALID, "bmo_psf_ee: bad argument (null pointer, n <= 0, n_planes <= 0, n_radii <= 0, n_hits < 0)");
    std::vector<double> thr;
    if (!ee_args_ok(shape, radii, n_radii, centers, n_planes, thr))
        return fail(BMO_ERR_INVALID, "bmo_psf_ee: shape must be 0 or 1, every radius finite and >= 0, every centre finite");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_ee", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    const int64_t n_pairs = (int64_t)n_planes * n_radii;
    if (n_hits == 0) {  // the sums of an image of zeros: the centroid is 0 / 0
        std::fill(ee, ee + n_pairs, std::nan(""));
        std::fill(energy, energy + n_pairs, 0.0);
        std::fill(sums, sums + n_planes, 0.0);
        for (int64_t q = 0; q < 2 * (int64_t)n_planes; ++q) centers_out[q] = centers ? centers[q] : std::nan("");
        if (out_intensity) std::fill(out_intensity, out_intensity + n_out, 0.0);
        return BMO_OK;
    }
    const int64_t n_rowsums = n_pairs * n, n_rowmoms = (int64_t)n_planes * n;
    if ((n_rowsums + 255) / 256 > (int64_t)0x7fffffff) return fail(BMO_ERR_LIMIT, "bmo_psf_ee: more row sums than one launch holds");
    hipStream_t st = 0;
    DevBuf d_int, d_field, d_rowmom, d_rowsum, d_cen, d_ee, d_energy, d_sums;
    Packed up;
    const size_t o_xs = up.add(xs, (size_t)n), o_zs = up.add(zs, (size_t)n), o_thr = up.add(thr);
    const size_t o_cen = centers ? up.add(centers, (size_t)n_planes * 2) : 0;
    int rc;
    if ((rc = up.upload(st)) || (rc = d_rowmom.alloc((size_t)n_rowmoms * sizeof(double2))) || (rc = d_rowsum.alloc((size_t)n_rowsums * 8)) ||
        (rc = d_cen.alloc((size_t)n_planes * sizeof(double2))) || (rc = d_ee.alloc((size_t)n_pairs * 8)) || (rc = d_energy.alloc((size_t)n_pairs * 8)) ||
        (rc = d_sums.alloc((size_t)n_planes * 8)))
        return rc;
    EventTimer timer;
    if ((rc = psf_focus_stack(hits, n_hits, origin, e1, e2, displacements, n_planes, xs, zs, n, false, d_int, d_field, timer, kernel_ms))) return rc;
    hipLaunchKernelGGL(psf_ee_moment_rows_kernel, dim3((unsigned)((n_rowmoms + 255) / 256)), dim3(256), 0, st, (const double*)d_int.p, up.at<double>(o_xs), n, n_rowmoms,
                       (double2*)d_rowmom.p);
    hipLaunchKernelGGL(psf_ee_moment_cols_kernel, dim3((unsigned)((n_planes + 255) / 256)), dim3(256), 0, st, (const double2*)d_rowmom.p, up.at<double>(o_zs), n, n_planes,
                       centers ? up.at<double2>(o_cen) : nullptr, (double*)d_sums.p, (double2*)d_cen.p);
    hipLaunchKernelGGL(psf_ee_rows_kernel, dim3((unsigned)((n_rowsums + 255) / 256)), dim3(256), 0, st, (const double*)d_int.p, up.at<double>(o_xs), up.at<double>(o_zs), n,
                       (const double2*)d_cen.p, shape, up.at<double>(o_thr), n_radii, n_rowsums, (double*)d_rowsum.p);
    hipLaunchKernelGGL(psf_ee_cols_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, (const double*)d_rowsum.p, n, n_radii, n_pairs, (const double*)d_sums.p,
                       (double*)d_ee.p, (double*)d_energy.p);
    if ((rc = timer.stop(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(ee, d_ee.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(energy, d_energy.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(centers_out, d_cen.p, (size_t)n_planes * sizeof(double2), hipMemcpyDeviceToHost));
    if (out_intensity) HIP_TRY(hipMemcpy(out_intensity, d_int.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return BMO_OK;
}

// The counts [K][n_radii] of the K = R.count.size() configurations from the device rows `rows` [..][cols]: centers [K][2].
static int spot_ee_read(const double* rows, int32_t cols, const Ranges& R, const double* centers, int32_t shape, const std::vector<double>& thr, int64_t* inside,
                        double* kernel_ms, const char* who) {
    const size_t K = R.count.size();
    const int32_t n_radii = (int32_t)thr.size();
    hipStream_t st = 0;
    const SplitPlan plan = rows_plan(R);
    unsigned n_items = 0;
    if (int rc = rows_items(plan, who, n_items)) return rc;
    std::vector<int32_t> perm((size_t)n_radii);  // sorted place s holds the caller's radius perm[s]
    for (int32_t k = 0; k < n_radii; ++k) perm[(size_t)k] = k;
    std::stable_sort(perm.begin(), perm.end(), [&](int32_t a, int32_t b) { return thr[(size_t)a] < thr[(size_t)b]; });
    std::vector<double> sorted((size_t)n_radii);
    for (int32_t s = 0; s < n_radii; ++s) sorted[(size_t)s] = thr[(size_t)perm[(size_t)s]];
    Packed up;
    const size_t o_work = up.add(plan.work), o_cen = up.add(centers, K * 2), o_thr = up.add(sorted), o_perm = up.add(perm);
    const size_t hist_bytes = K * (size_t)(n_radii + 1) * 8, out_bytes = K * (size_t)n_radii * 8;
    DevBuf d_hist, d_inside;
    int rc;
    if ((rc = up.upload(st)) || (rc = d_hist.alloc(hist_bytes)) || (rc = d_inside.alloc(out_bytes))) return rc;
    EventTimer timer;
    if ((rc = timer.start(st))) return rc;
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, hist_bytes, st));
    if (n_items > 0)
        hipLaunchKernelGGL(spot_ee_kernel, dim3(n_items), dim3(256), 0, st, rows, cols, up.at<SplitWork>(o_work), up.at<double2>(o_cen), shape, up.at<double>(o_thr), n_radii,
                           (unsigned long long*)d_hist.p);
    hipLaunchKernelGGL(spot_ee_cumulate_kernel, dim3((unsigned)K), dim3(256), 0, st, (const unsigned long long*)d_hist.p, up.at<int32_t>(o_perm), n_radii,
                       (long long*)d_inside.p);
    if ((rc = timer.stop(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(inside, d_inside.p, out_bytes, hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_spot_ee(const double* rows, int64_t n_rows, int32_t row_cols, int32_t rows_on_device, const double center[2], int32_t shape, const double* radii,
                           int32_t n_radii, int32_t device, int64_t* inside, double* kernel_ms) {
    if (!center || !radii || !inside || n_radii <= 0 || n_rows < 0 || (n_rows > 0 && !rows) || row_cols < 2 || row_cols > 9)
        return fail(BMO_ERR_INVALID, "bmo_spot_ee: bad argument (null pointer, n_radii <= 0, n_rows < 0, row_cols outside 2..9)");
    std::vector<double> thr;
    if (!ee_args_ok(shape, radii, n_radii, center, 1, thr))
        return fail(BMO_ERR_INVALID, "bmo_spot_ee: shape must be 0 or 1, every radius finite and >= 0, the centre finite");
    if (n_radii > SPOT_EE_MAX_RADII) return fail(BMO_ERR_LIMIT, "bmo_spot_ee: more than 4096 radii; ask for them in several calls");
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_rows;
    if (int rc = single_rows("bmo_spot_ee", rows, n_rows, row_cols, rows_on_device, device, d_rows)) return rc;
    return spot_ee_read(rows, row_cols, Ranges{{0}, {n_rows}}, center, shape, thr, inside, kernel_ms, "bmo_spot_ee");
}

extern "C" int bmo_spot_ee_sweep(bmo_trace_result* res, int32_t detector, int32_t n_configs, const double* centers, int32_t shape, const double* radii, int32_t n_radii,
                                 int64_t* inside, int64_t* n_rows, double* kernel_ms) {
    if (!res || !centers || !radii || !inside || !n_rows || n_radii <= 0)
        return fail(BMO_ERR_INVALID, "bmo_spot_ee_sweep: bad argument (null pointer, n_radii <= 0)");
    if (int rc = slot_check("bmo_spot_ee_sweep", res, detector, BMO_OBJ_SPOTDETECTOR, true, n_configs)) return rc;
    std::vector<double> thr;
    if (!ee_args_ok(shape, radii, n_radii, centers, n_configs, thr))
        return fail(BMO_ERR_INVALID, "bmo_spot_ee_sweep: shape must be 0 or 1, every radius finite and >= 0, every centre finite");
    if (n_radii > SPOT_EE_MAX_RADII) return fail(BMO_ERR_LIMIT, "bmo_spot_ee_sweep: more than 4096 radii; ask for them in several calls");
    if (kernel_ms) *kernel_ms = 0.0;
    const int64_t H = res->det_count[detector];
    if (H == 0) {  // every configuration reads like a call with n_rows = 0
        std::fill(inside, inside + (size_t)n_configs * (size_t)n_radii, (int64_t)0);
        std::fill(n_rows, n_rows + n_configs, (int64_t)0);
        return BMO_OK;
    }
    Ranges R;
    const double* rows;
    if (int rc = resident_rows("bmo_spot_ee_sweep", res, detector, H, n_configs, R, rows)) return rc;
    std::copy(R.count.begin(), R.count.end(), n_rows);
    return spot_ee_read(rows, 9, R, centers, shape, thr, inside, kernel_ms, "bmo_spot_ee_sweep");
}

// ====================================================================================================================
// Polychromatic read-out (include/bmo.h "Polychromatic read-out"): the rows of a slot split by wave number into band-contiguous ranges,
// which every single-call read-out above then reads through its hits_on_device pointer, and the weighted sum of the bands' stacks.
//
// Discovery (ks == NULL): one pass over column 8.  A wave usually agrees on one key: every lane compares its key with the first pending
// lane's, the ballot's popcount is that key's count, one lane adds it to a table in LDS, and the loop goes on with the lanes that
// disagreed.  The workgroup's table is merged into a global open-addressed table of 64-bit patterns (atomicCAS on the key, an integer
// atomic add on the count); a table that is full raises a flag.  The host sorts.  Integer counts of a set: no order shows in the result.
//
// Stable partition, three launches over tiles of PSF_TILE rows:
//   (a) psf_band_count_kernel: every row is classified against the <= 64 keys in LDS; the rows of each (band, tile) are counted by ballot
//       and popcount per wave, the four waves folded through LDS;
//   (b) psf_band_scan_kernel: one workgroup per band, the exclusive scan of the band's tile counts and the band's total;
//   (c) psf_band_scatter_kernel: classifies again; a row's place is base[band] + scan[band][tile] + the count of the earlier waves of the
//       tile + the lanes of the wave below it in the same band.  No atomic decides a position: the order is fixed by construction.
// The scatter writes every row straight to its place (nine stores of 8 bytes per lane).
struct bmo_psf_bands {
    int32_t device = 0;
    int64_t n_rows = 0, unmatched = 0;  // matched (the sum of `count`) and dropped rows
    std::vector<double> ks;
    std::vector<int64_t> base, count;  // band b: rows base[b] .. base[b] + count[b] - 1 of `rows`
    DevBuf rows;                       // [n_rows][9], band-major
};

namespace {

constexpr int BAND_LDS_SLOTS = 128, BAND_TABLE_SLOTS = 256;  // powers of two, at least twice BMO_PSF_MAX_BANDS
constexpr unsigned long long BAND_EMPTY = ~0ull;              // a NaN's pattern: never a key
static_assert(BAND_LDS_SLOTS >= 2 * BMO_PSF_MAX_BANDS && BAND_TABLE_SLOTS >= 2 * BMO_PSF_MAX_BANDS && BMO_PSF_MAX_BANDS <= 64, "band tables");

struct BandTable {
    unsigned long long keys[BAND_TABLE_SLOTS], counts[BAND_TABLE_SLOTS];
    unsigned long long n_nan, overflow;
};

// `cnt` more rows of `key` in the open-addressed table (keys, counts) of `slots` entries; false: the table holds `slots` other keys
__device__ __forceinline__ bool band_table_add(unsigned long long* keys, unsigned long long* counts, int slots, unsigned long long key, unsigned long long cnt) {
    unsigned s = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 40) & (unsigned)(slots - 1);
    for (int probe = 0; probe < slots; ++probe, s = (s + 1) & (unsigned)(slots - 1)) {
        const unsigned long long prev = atomicCAS(&keys[s], BAND_EMPTY, key);
        if (prev == BAND_EMPTY || prev == key) {
            atomicAdd(&counts[s], cnt);
            return true;
        }
    }
    return false;
}

// workgroup blockIdx.x reads tiles blockIdx.x, blockIdx.x + gridDim.x, ... of column 8
__global__ __launch_bounds__(256) void psf_band_discover_kernel(const double* __restrict__ hits, int64_t n_hits, int64_t n_tiles, BandTable* __restrict__ table) {
    __shared__ unsigned long long l_keys[BAND_LDS_SLOTS], l_counts[BAND_LDS_SLOTS], l_nan, l_over;
    for (int q = threadIdx.x; q < BAND_LDS_SLOTS; q += 256) l_keys[q] = BAND_EMPTY, l_counts[q] = 0;
    if (threadIdx.x == 0) l_nan = 0, l_over = 0;
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t h = tile * PSF_TILE + threadIdx.x;
        const bool in = h < n_hits;
        double k = in ? hits[h * 9 + 8] : 0.0;
        if (k == 0.0) k = 0.0;  // -0 == +0: one key
        const bool nan = in && k != k;
        const unsigned long long m_nan = __ballot(nan);
        if (m_nan && lane_id() == 0) atomicAdd(&l_nan, (unsigned long long)__popcll(m_nan));
        bool pending = in && !nan;
        for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {  // one trip per distinct key of the wave
            const int leader = __ffsll(todo) - 1;
            const double k0 = __shfl(k, leader);
            const bool same = pending && k == k0;
            const unsigned long long m = __ballot(same);
            if (lane_id() == leader && !band_table_add(l_keys, l_counts, BAND_LDS_SLOTS, (unsigned long long)__double_as_longlong(k0), (unsigned long long)__popcll(m)))
                atomicAdd(&l_over, 1ull);
            pending = pending && !same;
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < BAND_LDS_SLOTS; q += 256)
        if (l_keys[q] != BAND_EMPTY && !band_table_add(table->keys, table->counts, BAND_TABLE_SLOTS, l_keys[q], l_counts[q])) atomicAdd(&table->overflow, 1ull);
    if (threadIdx.x == 0) {
        if (l_nan) atomicAdd(&table->n_nan, l_nan);
        if (l_over) atomicAdd(&table->overflow, l_over);
    }
}

constexpr int BAND_SLOTS = BMO_PSF_MAX_BANDS + 1;  // the bands and, at index n_bands, the rows of none

// Row tile * PSF_TILE + threadIdx.x classified against the n_bands keys: its band, n_bands for a row of none (a NaN compares false), -1 for
// a lane past the rows.  wcount[wave][band] (zeroed by the caller) receives the wave's rows of every band it holds, `rank` the lanes of the
// wave below this one in the same band.  Every lane of the workgroup calls it.
__device__ __forceinline__ int band_classify_tile(const double* __restrict__ hits, int64_t n_hits, int64_t tile, const double* keys, int n_bands,
                                                  int (*wcount)[BAND_SLOTS], int& rank) {
    const int64_t h = tile * PSF_TILE + threadIdx.x;
    int band = -1;
    if (h < n_hits) {
        const double k = hits[h * 9 + 8];
        band = n_bands;
        for (int b = 0; b < n_bands; ++b)
            if (k == keys[b]) band = b;  // the keys are distinct: at most one compares equal
    }
    rank = 0;
    bool pending = band >= 0;
    for (unsigned long long todo = __ballot(pending); todo; todo = __ballot(pending)) {  // one trip per distinct band of the wave
        const int leader = __ffsll(todo) - 1;
        const int b0 = __shfl(band, leader);
        const bool same = pending && band == b0;
        const unsigned long long m = __ballot(same);
        if (same) rank = prefix_rank(m);
        if (lane_id() == leader) wcount[threadIdx.x >> 6][b0] = __popcll(m);
        pending = pending && !same;
    }
    return band;
}

// the keys into LDS and the wave counts zeroed; the caller syncs
__device__ __forceinline__ void band_tile_begin(const double* __restrict__ keys_g, int n_bands, double* keys, int (*wcount)[BAND_SLOTS]) {
    if ((int)threadIdx.x < n_bands) keys[threadIdx.x] = keys_g[threadIdx.x];
    for (int q = threadIdx.x; q < 4 * BAND_SLOTS; q += 256) wcount[q / BAND_SLOTS][q % BAND_SLOTS] = 0;
}

// (a) tile blockIdx.x: tile_count[band][tile], band = 0 .. n_bands (the last: the rows of no band)
__global__ __launch_bounds__(256) void psf_band_count_kernel(const double* __restrict__ hits, int64_t n_hits, const double* __restrict__ keys_g, int n_bands,
                                                             int64_t n_tiles, int32_t* __restrict__ tile_count) {
    __shared__ double keys[BMO_PSF_MAX_BANDS];
    __shared__ int wcount[4][BAND_SLOTS];
    band_tile_begin(keys_g, n_bands, keys, wcount);
    __syncthreads();
    int rank;
    (void)band_classify_tile(hits, n_hits, blockIdx.x, keys, n_bands, wcount, rank);
    __syncthreads();
    const int b = threadIdx.x;
    if (b <= n_bands) tile_count[(int64_t)b * n_tiles + blockIdx.x] = (wcount[0][b] + wcount[1][b]) + (wcount[2][b] + wcount[3][b]);
}

// (b) band blockIdx.x: tile_start[band][tile] = the rows of the band in the tiles before, totals[band] = its rows.  Lane l owns a run of
// consecutive tiles.
__global__ __launch_bounds__(256) void psf_band_scan_kernel(const int32_t* __restrict__ tile_count, int64_t n_tiles, int64_t* __restrict__ tile_start,
                                                            int64_t* __restrict__ totals) {
    __shared__ int64_t run_start[256];
    const int32_t* c = tile_count + (int64_t)blockIdx.x * n_tiles;
    int64_t* s = tile_start + (int64_t)blockIdx.x * n_tiles;
    const int64_t per = (n_tiles + 255) / 256;
    const int64_t t0 = std::min<int64_t>((int64_t)threadIdx.x * per, n_tiles), t1 = std::min<int64_t>(t0 + per, n_tiles);
    int64_t sum = 0;
    for (int64_t t = t0; t < t1; ++t) sum += c[t];
    run_start[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int q = 0; q < 256; ++q) {
            const int64_t v = run_start[q];
            run_start[q] = acc;
            acc += v;
        }
        totals[blockIdx.x] = acc;
    }
    __syncthreads();
    int64_t at = run_start[threadIdx.x];
    for (int64_t t = t0; t < t1; ++t) {
        s[t] = at;
        at += c[t];
    }
}

// (c) tile blockIdx.x: every matched row copied to its place in `out` [n_out][9]
__global__ __launch_bounds__(256) void psf_band_scatter_kernel(const double* __restrict__ hits, int64_t n_hits, const double* __restrict__ keys_g, int n_bands,
                                                               int64_t n_tiles, const int64_t* __restrict__ tile_start, const int64_t* __restrict__ totals,
                                                               int64_t n_out, double* __restrict__ out) {
    __shared__ double keys[BMO_PSF_MAX_BANDS];
    __shared__ int wcount[4][BAND_SLOTS];
    __shared__ int64_t base[BMO_PSF_MAX_BANDS];
    band_tile_begin(keys_g, n_bands, keys, wcount);
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int b = 0; b < n_bands; ++b) {
            base[b] = acc;
            acc += totals[b];
        }
    }
    __syncthreads();
    int rank;
    const int band = band_classify_tile(hits, n_hits, blockIdx.x, keys, n_bands, wcount, rank);
    __syncthreads();
    if (band < 0 || band >= n_bands) return;
    int before = 0;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += wcount[w][band];
    const int64_t dst = base[band] + tile_start[(int64_t)band * n_tiles + blockIdx.x] + before + rank;
    if (dst >= n_out) return;  // (cannot happen: the totals are the counts of the same classification)
    const double* r = hits + ((int64_t)blockIdx.x * PSF_TILE + threadIdx.x) * 9;
    double* o = out + dst * 9;
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = r[q];
}

// acc = c * I (first) or acc + c * I per sample, a multiply and an add; src nullptr: a band without rows, I = 0
__global__ void psf_poly_combine_kernel(double* __restrict__ acc, const double* __restrict__ src, double c, int first, int64_t n_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const double v = c * (src ? src[i] : 0.0);
    acc[i] = first ? v : acc[i] + v;
}

}  // namespace

// The distinct keys of column 8 of the n_hits > 0 device rows, ascending, with their counts; n_nan: the rows whose key is a NaN.
static int psf_bands_discover(const double* hits, int64_t n_hits, hipStream_t st, std::vector<double>& ks, std::vector<int64_t>& counts, int64_t& n_nan) {
    std::unique_ptr<BandTable> host(new BandTable);
    std::fill(host->keys, host->keys + BAND_TABLE_SLOTS, BAND_EMPTY);
    std::fill(host->counts, host->counts + BAND_TABLE_SLOTS, 0ull);
    host->n_nan = host->overflow = 0;
    DevBuf d_table;
    if (int rc = d_table.alloc(sizeof(BandTable))) return rc;
    HIP_TRY(hipMemcpyAsync(d_table.p, host.get(), sizeof(BandTable), hipMemcpyHostToDevice, st));
    const int64_t n_tiles = (n_hits + PSF_TILE - 1) / PSF_TILE;
    hipLaunchKernelGGL(psf_band_discover_kernel, dim3((unsigned)std::min<int64_t>(n_tiles, 1024)), dim3(256), 0, st, hits, n_hits, n_tiles, (BandTable*)d_table.p);
    HIP_TRY(hipMemcpyAsync(host.get(), d_table.p, sizeof(BandTable), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    std::vector<std::pair<double, int64_t>> found;
    for (int q = 0; q < BAND_TABLE_SLOTS; ++q)
        if (host->keys[q] != BAND_EMPTY) {
            double k;
            memcpy(&k, &host->keys[q], 8);
            found.push_back({k, (int64_t)host->counts[q]});
        }
    if (host->overflow != 0 || found.size() > (size_t)BMO_PSF_MAX_BANDS)
        return fail(BMO_ERR_LIMIT, "bmo_psf_bands_create: the rows hold more than BMO_PSF_MAX_BANDS (64) distinct wave numbers");
    std::sort(found.begin(), found.end());
    for (const auto& f : found) ks.push_back(f.first), counts.push_back(f.second);
    n_nan = (int64_t)host->n_nan;
    return BMO_OK;
}

extern "C" int bmo_psf_bands_create(const double* hits, int64_t n_hits, int32_t hits_on_device, int32_t device, const double* ks, int32_t n_ks, bmo_psf_bands** out,
                                    double* kernel_ms) {
    if (!out || n_hits < 0 || (n_hits > 0 && !hits)) return fail(BMO_ERR_INVALID, "bmo_psf_bands_create: bad argument (null pointer, n_hits < 0)");
    if (ks) {
        if (n_ks <= 0) return fail(BMO_ERR_INVALID, "bmo_psf_bands_create: ks given with n_ks <= 0");
        for (int32_t a = 0; a < n_ks; ++a) {
            if (!std::isfinite(ks[a])) return fail(BMO_ERR_INVALID, "bmo_psf_bands_create: a wave number of ks is not finite");
            for (int32_t b = 0; b < a && b < BMO_PSF_MAX_BANDS; ++b)
                if (ks[a] == ks[b]) return fail(BMO_ERR_INVALID, "bmo_psf_bands_create: two wave numbers of ks are equal");
        }
        if (n_ks > BMO_PSF_MAX_BANDS) return fail(BMO_ERR_LIMIT, "bmo_psf_bands_create: more than BMO_PSF_MAX_BANDS (64) bands");
    }
    if (kernel_ms) *kernel_ms = 0.0;
    DevBuf d_hits;
    if (int rc = single_rows("bmo_psf_bands_create", hits, n_hits, 9, hits_on_device, device, d_hits)) return rc;
    const int64_t n_tiles = (n_hits + PSF_TILE - 1) / PSF_TILE;
    if (n_tiles > (int64_t)0x7fffffff) return fail(BMO_ERR_LIMIT, "bmo_psf_bands_create: more tiles of rows than one launch holds");
    std::unique_ptr<bmo_psf_bands> B(new bmo_psf_bands);
    B->device = device;
    if (ks) B->ks.assign(ks, ks + n_ks);
    hipStream_t st = 0;
    EventTimer timer;
    std::vector<int64_t> found;  // the counts the discovery pass saw
    int64_t n_nan = 0;
    if (n_hits > 0)
        if (int rc = timer.start(st)) return rc;
    if (!ks && n_hits > 0)
        if (int rc = psf_bands_discover(hits, n_hits, st, B->ks, found, n_nan)) return rc;
    const int nb = (int)B->ks.size();
    B->base.assign((size_t)nb, 0);
    B->count.assign((size_t)nb, 0);
    if (n_hits == 0 || nb == 0) {  // nothing to place: every row, if any, has a NaN key
        B->unmatched = n_nan;
        if (int rc = B->rows.alloc(0)) return rc;
        if (n_hits > 0)
            if (int rc = timer.stop(kernel_ms)) return rc;
        *out = B.release();
        return BMO_OK;
    }
    Packed up;
    const size_t o_keys = up.add(B->ks);
    DevBuf d_count, d_start, d_totals;
    int rc;
    if ((rc = up.upload(st)) || (rc = d_count.alloc((size_t)(nb + 1) * (size_t)n_tiles * 4)) || (rc = d_start.alloc((size_t)(nb + 1) * (size_t)n_tiles * 8)) ||
        (rc = d_totals.alloc((size_t)(nb + 1) * 8)))
        return rc;
    hipLaunchKernelGGL(psf_band_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, hits, n_hits, up.at<double>(o_keys), nb, n_tiles, (int32_t*)d_count.p);
    hipLaunchKernelGGL(psf_band_scan_kernel, dim3((unsigned)(nb + 1)), dim3(256), 0, st, (const int32_t*)d_count.p, n_tiles, (int64_t*)d_start.p, (int64_t*)d_totals.p);
    std::vector<int64_t> totals((size_t)nb + 1);
    HIP_TRY(hipMemcpyAsync(totals.data(), d_totals.p, totals.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    int64_t matched = 0;
    for (int b = 0; b < nb; ++b) {
        B->base[(size_t)b] = matched;
        B->count[(size_t)b] = totals[(size_t)b];
        matched += totals[(size_t)b];
    }
    B->n_rows = matched;
    B->unmatched = totals[(size_t)nb];
    if (matched + B->unmatched != n_hits || (!ks && (B->count != found || B->unmatched != n_nan)))
        return fail(BMO_ERR_INTERNAL, "bmo_psf_bands_create: the band counts do not add up to the rows");
    if ((rc = B->rows.alloc((size_t)matched * 9 * sizeof(double)))) return rc;
    if (matched > 0)
        hipLaunchKernelGGL(psf_band_scatter_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, hits, n_hits, up.at<double>(o_keys), nb, n_tiles, (const int64_t*)d_start.p,
                           (const int64_t*)d_totals.p, matched, (double*)B->rows.p);
    if ((rc = timer.stop(kernel_ms))) return rc;
    *out = B.release();
    return BMO_OK;
}

extern "C" int bmo_psf_bands_info(const bmo_psf_bands* b, int32_t* n_bands, int64_t* n_rows, int64_t* unmatched, int32_t* device) {
    if (!b) return fail(BMO_ERR_INVALID, "bmo_psf_bands_info: null handle");
    if (n_bands) *n_bands = (int32_t)b->ks.size();
    if (n_rows) *n_rows = b->n_rows;
    if (unmatched) *unmatched = b->unmatched;
    if (device) *device = b->device;
    return BMO_OK;
}

extern "C" int bmo_psf_bands_get(const bmo_psf_bands* b, int32_t band, double* k, const double** rows, int64_t* count) {
    if (!b) return fail(BMO_ERR_INVALID, "bmo_psf_bands_get: null handle");
    if (band < 0 || (size_t)band >= b->ks.size()) return fail(BMO_ERR_INVALID, "bmo_psf_bands_get: band index out of range");
    if (k) *k = b->ks[(size_t)band];
    if (rows) *rows = (const double*)b->rows.p + 9 * b->base[(size_t)band];
    if (count) *count = b->count[(size_t)band];
    return BMO_OK;
}

extern "C" int bmo_psf_bands_free(bmo_psf_bands* b) {
    delete b;
    return BMO_OK;
}

// what the two polychromatic entries refuse of their coefficients
static bool poly_coeffs_ok(const bmo_psf_bands* b, const double* coeffs) {
    for (size_t q = 0; q < b->ks.size(); ++q)
        if (!std::isfinite(coeffs[q])) return false;
    return true;
}

// The weighted sum of the bands' stacks, left on the device: d_acc [n_planes][n * n] (at least one band).  Band after band: psf_focus_stack
// on the band's range, then the combine launch, so one band's stack and the accumulator are held; out_band (host, [n_bands][n_out]) takes
// each band's stack as it is made.  `timer` runs from the first launch; the caller may queue more on stream 0 and stop it again.
static int psf_poly_stack(const bmo_psf_bands* B, const double* origin, const double* e1, const double* e2, const double* disp, int32_t n_planes, const double* xs,
                          const double* zs, int32_t n, const double* coeffs, DevBuf& d_acc, double* out_band, EventTimer& timer, double* kernel_ms) {
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    hipStream_t st = 0;
    if (int rc = d_acc.alloc(n_out * sizeof(double))) return rc;
    for (size_t b = 0; b < B->ks.size(); ++b) {
        DevBuf d_int, d_field;
        const double* src = nullptr;
        if (B->count[b] > 0) {
            if (int rc = psf_focus_stack((const double*)B->rows.p + 9 * B->base[b], B->count[b], origin, e1, e2, disp, n_planes, xs, zs, n, false, d_int, d_field, timer, kernel_ms))
                return rc;
            src = (const double*)d_int.p;
        }
        if (!timer.e0)
            if (int rc = timer.start(st)) return rc;
        hipLaunchKernelGGL(psf_poly_combine_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, (double*)d_acc.p, src, coeffs[b], b == 0 ? 1 : 0, (int64_t)n_out);
        if (out_band) {
            if (src) HIP_TRY(hipMemcpy(out_band + b * n_out, src, n_out * sizeof(double), hipMemcpyDeviceToHost));
            else std::fill(out_band + b * n_out, out_band + (b + 1) * n_out, 0.0);
        }
    }
    return timer.stop(kernel_ms);
}

extern "C" int bmo_psf_poly_through_focus(const bmo_psf_bands* b, const double origin[3], const double e1[3], const double e2[3], const double* displacements,
                                          int32_t n_planes, const double* xs, const double* zs, int32_t n, const double* coeffs, double* out_intensity,
                                          double* out_band_intensity, double* kernel_ms) {
    if (!b || !origin || !e1 || !e2 || !displacements || !xs || !zs || !coeffs || !out_intensity || n <= 0 || n_planes <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_poly_through_focus: bad argument (null pointer, n <= 0, n_planes <= 0)");
    if (!poly_coeffs_ok(b, coeffs)) return fail(BMO_ERR_INVALID, "bmo_psf_poly_through_focus: a coefficient is not finite");
    if (kernel_ms) *kernel_ms = 0.0;
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    if (b->ks.empty()) {
        std::fill(out_intensity, out_intensity + n_out, 0.0);
        return BMO_OK;
    }
    if ((n_out + 255) / 256 > (size_t)0x7fffffff) return fail(BMO_ERR_LIMIT, "bmo_psf_poly_through_focus: more samples than one launch holds");
    HIP_TRY(hipSetDevice(b->device));
    DevBuf d_acc;
    EventTimer timer;
    if (int rc = psf_poly_stack(b, origin, e1, e2, displacements, n_planes, xs, zs, n, coeffs, d_acc, out_band_intensity, timer, kernel_ms)) return rc;
    HIP_TRY(hipMemcpy(out_intensity, d_acc.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return BMO_OK;
}

extern "C" int bmo_psf_poly_otf(const bmo_psf_bands* b, const double origin[3], const double e1[3], const double e2[3], const double* displacements, int32_t n_planes,
                                const double* xs, const double* zs, int32_t n, const double* coeffs, const double* freqs, int32_t n_freqs, double* otf, double* mtf,
                                double* sums, double* out_intensity, double* kernel_ms) {
    if (!b || !origin || !e1 || !e2 || !displacements || !xs || !zs || !coeffs || !freqs || !otf || !mtf || !sums || n <= 0 || n_planes <= 0 || n_freqs <= 0)
        return fail(BMO_ERR_INVALID, "bmo_psf_poly_otf: bad argument (null pointer, n <= 0, n_planes <= 0, n_freqs <= 0)");
    if (!poly_coeffs_ok(b, coeffs)) return fail(BMO_ERR_INVALID, "bmo_psf_poly_otf: a coefficient is not finite");
    if (!otf_freqs_ok(freqs, n_freqs)) return fail(BMO_ERR_INVALID, "bmo_psf_poly_otf: a frequency is not finite");
    if (kernel_ms) *kernel_ms = 0.0;
    const size_t n_out = (size_t)n_planes * (size_t)n * (size_t)n;
    const int64_t n_pairs = (int64_t)n_planes * n_freqs;
    if (b->ks.empty() || b->n_rows == 0) {
        otf_fill_empty((size_t)n_pairs, (size_t)n_planes, otf, mtf, sums);
        if (out_intensity) std::fill(out_intensity, out_intensity + n_out, 0.0);
        return BMO_OK;
    }
    const int64_t n_rowsums = (int64_t)n_planes * (n_freqs + 1) * n;
    if ((n_rowsums + 255) / 256 > (int64_t)0x7fffffff || (n_out + 255) / 256 > (size_t)0x7fffffff)
        return fail(BMO_ERR_LIMIT, "bmo_psf_poly_otf: more row sums or samples than one launch holds");
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t st = 0;
    DevBuf d_acc, d_rowsum, d_otf, d_mtf, d_sums;
    Packed up;
    const size_t o_xs = up.add(xs, (size_t)n), o_zs = up.add(zs, (size_t)n), o_freq = up.add(freqs, (size_t)n_freqs * 2);
    int rc;
    if ((rc = up.upload(st)) || (rc = d_rowsum.alloc((size_t)n_rowsums * sizeof(double2))) || (rc = d_otf.alloc((size_t)n_pairs * sizeof(double2))) ||
        (rc = d_mtf.alloc((size_t)n_pairs * 8)) || (rc = d_sums.alloc((size_t)n_planes * 8)))
        return rc;
    EventTimer timer;
    if ((rc = psf_poly_stack(b, origin, e1, e2, displacements, n_planes, xs, zs, n, coeffs, d_acc, nullptr, timer, kernel_ms))) return rc;
    hipLaunchKernelGGL(psf_otf_rows_kernel, dim3((unsigned)((n_rowsums + 255) / 256)), dim3(256), 0, st, (const double*)d_acc.p, up.at<double>(o_xs), n,
                       up.at<double2>(o_freq), n_freqs, n_rowsums, (double2*)d_rowsum.p);
    hipLaunchKernelGGL(psf_otf_cols_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, (const double2*)d_rowsum.p, up.at<double>(o_zs), n,
                       up.at<double2>(o_freq), n_freqs, n_pairs, (double2*)d_otf.p, (double*)d_mtf.p, (double*)d_sums.p);
    if ((rc = timer.stop(kernel_ms))) return rc;
    HIP_TRY(hipMemcpy(otf, d_otf.p, (size_t)n_pairs * sizeof(double2), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mtf, d_mtf.p, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sums, d_sums.p, (size_t)n_planes * 8, hipMemcpyDeviceToHost));
    if (out_intensity) HIP_TRY(hipMemcpy(out_intensity, d_acc.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return BMO_OK;
}
