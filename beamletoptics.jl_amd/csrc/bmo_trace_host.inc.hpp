// bmo_trace_host.inc.hpp — host side of one trace (included by bmo_engine.hip inside its anonymous namespace; shares its pools, error helpers
// and kernels).  run_trace at the end is the driver; everything above it is one phase of a solve, given what it needs as arguments, with the
// helper kernels it launches right above it:
//   build_retrace_tables  the OldSolution tables of the solution a retrace re-walks (old_obj_scatter_kernel, old_first_child_kernel)
//   device_ctx            stream, events and pinned counters of a device, made once
//   NodeTable             the node arrays of a solution: allocation, growth, the kernels' view of them
//   ChunkArena            the segment log's storage: chunks bumped out of large blocks, rewound behind a launch
//   select_step_kernels   the step kernels of a beam kind / scene level / fresh, retrace or sweep solve
//   plan_launch, fill_step_params, tile_order_feedback, build_sweep_lane_map, print_timeline, launch_step: the parts of one launch
//   order_nodes, count_and_gather_hits               the canonical node order, the segment count and the detector tables behind the last launch
//   step_once, finish_solve                          one turn of the step loop; everything behind the loop, behind ONE synchronisation

// ---- the retrace tables of a finished solution (OldSolution), built when it is first retraced
__global__ void old_obj_scatter_kernel(Chunk c, int32_t chunk_index, const int32_t* __restrict__ rec_start, int32_t* __restrict__ rec_obj,
                                       int64_t* __restrict__ rec_loc) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.count) return;
    const int32_t node = chunk_node(c, j);
    if (node < 0) return;  // hole of a fused level
    const int32_t k = c.i[I_K * c.cap + j];
    rec_obj[(int64_t)rec_start[node] + k] = c.i[I_OBJ * c.cap + j];
    rec_loc[(int64_t)rec_start[node] + k] = ((int64_t)chunk_index << OLD_LOC_SHIFT) | j;
}
__global__ void old_first_child_kernel(const int32_t* __restrict__ parent, const unsigned long long* __restrict__ key, int64_t n, int32_t* __restrict__ first_child) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const int32_t p = parent[c];
    if (p >= 0 && !(key[c] & 1ull)) first_child[p] = (int32_t)c;  // transmitted child (path bit 0); the reflected one is c + 1
}
// OldSolution tables of `prev` (device arrays keyed by prev's node ids), built once per solution.
int build_retrace_tables(bmo_trace_result* prev, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(prev->rt_mu);
    if (!prev->has_log) return fail(BMO_ERR_INVALID, "retrace: the previous solution was solved with record_segments = 0 (no segment log to re-walk)");
    if (prev->rt_built) return BMO_OK;
    const int64_t nn = prev->n_nodes, nr = prev->n_records;
    if (nr >= (int64_t)1 << 31) return fail(BMO_ERR_UNSUPPORTED, "retrace: previous solution has more than 2^31 segments");
    int rc;
    if ((rc = prev->rt_rec_start.alloc((size_t)std::max<int64_t>(nn, 1) * 4)) || (rc = prev->rt_rec_obj.alloc((size_t)std::max<int64_t>(nr, 1) * 4)) ||
        (rc = prev->rt_first_child.alloc((size_t)std::max<int64_t>(nn, 1) * 4)) || (rc = prev->rt_rec_loc.alloc((size_t)std::max<int64_t>(nr, 1) * 8)) ||
        (rc = prev->rt_chunks.alloc(std::max<size_t>(prev->chunks.size(), 1) * sizeof(OldChunk))))
        return rc;
    if (prev->chunks.size() >= ((size_t)1 << (63 - OLD_LOC_SHIFT))) return fail(BMO_ERR_UNSUPPORTED, "retrace: previous solution has too many log chunks");
    if (nn > 0) {
        Temps tmp;
        CUB_TRY(tmp, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)prev->n_nseg.p, (int32_t*)prev->rt_rec_start.p, (int)nn, stream));
        std::vector<OldChunk> oc(prev->chunks.size());
        for (size_t q = 0; q < prev->chunks.size(); ++q) oc[q] = OldChunk{prev->chunks[q].d, prev->chunks[q].cap};
        if (!oc.empty()) HIP_TRY(hipMemcpyAsync(prev->rt_chunks.p, oc.data(), oc.size() * sizeof(OldChunk), hipMemcpyHostToDevice, stream));
        for (size_t q = 0; q < prev->chunks.size(); ++q) {
            const Chunk& c = prev->chunks[q];
            if (c.count > 0)
                hipLaunchKernelGGL(old_obj_scatter_kernel, dim3((unsigned)((c.count + 255) / 256)), dim3(256), 0, stream, c, (int32_t)q,
                                   (const int32_t*)prev->rt_rec_start.p, (int32_t*)prev->rt_rec_obj.p, (int64_t*)prev->rt_rec_loc.p);
        }
        HIP_TRY(hipMemsetAsync(prev->rt_first_child.p, 0xFF, (size_t)nn * 4, stream));
        hipLaunchKernelGGL(old_first_child_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, stream, (const int32_t*)prev->n_parent.p,
                           (const unsigned long long*)prev->n_key.p, nn, (int32_t*)prev->rt_first_child.p);
        HIP_TRY(hipStreamSynchronize(stream));  // tmp goes back to the pool
        HIP_TRY(hipGetLastError());
        if (dbg_on()) {
            const int q = (int)std::min<int64_t>(nn, 6), qr = (int)std::min<int64_t>(nr, 24);
            std::vector<int32_t> a(q), b(q), c(q), d(qr);
            (void)hipMemcpy(a.data(), prev->n_nseg.p, q * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(b.data(), prev->rt_rec_start.p, q * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(c.data(), prev->rt_first_child.p, q * 4, hipMemcpyDeviceToHost);
            (void)hipMemcpy(d.data(), prev->rt_rec_obj.p, qr * 4, hipMemcpyDeviceToHost);
            for (int i = 0; i < q; ++i) DBG("retrace table node %d: nseg %d rec_start %d first_child %d", i, a[i], b[i], c[i]);
            std::string line;
            for (int i = 0; i < qr; ++i) line += std::to_string(d[i]) + " ";
            DBG("retrace table rec_obj: %s", line.c_str());
        }
    }
    prev->rt_built = true;
    return BMO_OK;
}

// Everything a solve counts, in ONE device block: a solve sets it by one copy of the context's pinned image and reads it back by one copy
// behind the finish pass.  `ctr` comes first (StepParams::ctr; the read-back behind every launch takes these bytes alone), the 64
// call-counter shards lie 128 B apart (StepParams::call_shards), `det_off` holds the first row of every detector in the hit table and
// the number of rows behind them (written by hit_gather_kernel).  Word 1 of every shard's line counts segments (hit_count_kernel; the
// step kernels count calls in word 0).
constexpr int MAX_DETECTORS = 1023;  // hit_count_kernel / hit_gather_kernel keep a count per detector and wave in LDS
struct TailBlock {
    alignas(128) Counters ctr;
    alignas(128) unsigned long long shards[64 * 16];
    int32_t det_off[MAX_DETECTORS + 1];
};
inline size_t tail_bytes(int n_det) { return offsetof(TailBlock, det_off) + (size_t)(n_det + 1) * 4; }

// one trace stream + timing events per device, created once (hipStreamCreate costs ~1 ms)
struct DevCtx {
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    Counters* pinned = nullptr;
    TailBlock* tail_img = nullptr;   // pinned; all zero but ctr.node_count, which a solve sets to its root count before it copies the image
    TailBlock* tail_back = nullptr;  // pinned; the block as read back behind the finish pass
    std::vector<hipEvent_t> step_ev;
    std::mutex busy;  // one trace at a time per device: the stream, events and pinned counters are shared
};
int device_ctx(int device, DevCtx*& out) {
    static std::mutex ctx_mu;
    static std::vector<std::pair<int, std::unique_ptr<DevCtx>>> ctxs;
    std::lock_guard<std::mutex> lk(ctx_mu);
    for (auto& c : ctxs)
        if (c.first == device) {
            out = c.second.get();
            return BMO_OK;
        }
    auto nc = std::make_unique<DevCtx>();
    // non-blocking: no implicit synchronisation with the NULL stream, so a collective or copy another library has in flight
    // there (RCCL all-gather of the previous solve's hits) overlaps this solve
    HIP_TRY(hipStreamCreateWithFlags(&nc->stream, hipStreamNonBlocking));
    for (int q = 0; q < 4; ++q) HIP_TRY(hipEventCreate(&nc->ev[q]));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&nc->pinned), sizeof(Counters), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&nc->tail_img), 2 * sizeof(TailBlock), hipHostMallocDefault));
    std::memset(nc->tail_img, 0, 2 * sizeof(TailBlock));
    nc->tail_back = nc->tail_img + 1;
    out = nc.get();
    ctxs.emplace_back(device, std::move(nc));
    return BMO_OK;
}

// The node arrays of a solution.  `each` is the ONE list of them with their element sizes: allocation and growth walk it (a new array
// is added there and to NodeArrays).  n_hit holds 9 doubles per sub-beam; n_old exists in retraces only.
struct NodeTable {
    bmo_trace_result* R;
    int nsub;
    bool retrace;
    int64_t cap = 0;
    template <class F>
    int each(F&& f) const {
        using T = bmo_trace_result;
        const struct {
            DevBuf T::*buf;
            size_t elem;
        } cols[] = {{&T::n_root, 4},   {&T::n_parent, 4}, {&T::n_nseg, 4},   {&T::n_status, 4},          {&T::n_li, 4}, {&T::n_hitdet, 4},
                    {&T::n_key, 8},    {&T::n_lambda, 8}, {&T::n_hit, 72 * (size_t)nsub}, {&T::n_aux, 32}, {&T::n_old, retrace ? 4u : 0u}};
        for (const auto& c : cols)
            if (c.elem)
                if (int r = f(R->*c.buf, c.elem)) return r;
        return BMO_OK;
    }
    int alloc(int64_t n) {
        cap = n;
        return each([&](DevBuf& b, size_t elem) { return b.alloc((size_t)n * elem); });
    }
    // room for `need` nodes: max(need, 2 * cap), every array copied on the stream, the old block back to the pool at once
    int grow(int64_t need, hipStream_t stream) {
        if (need <= cap) return BMO_OK;
        const int64_t ncap = std::max(need, cap * 2);
        int r = each([&](DevBuf& b, size_t elem) -> int {
            DevBuf nb;
            if (int ra = nb.alloc((size_t)ncap * elem)) return ra;
            if (hipMemcpyAsync(nb.p, b.p, (size_t)cap * elem, hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail(BMO_ERR_NO_DEVICE, "grow nodes");
            (void)hipStreamSynchronize(stream);
            std::swap(b.p, nb.p);
            std::swap(b.bytes, nb.bytes);
            PoolHold::Now at_once;  // the old table goes back right away (the copy above has completed)
            nb.release();
            return BMO_OK;
        });
        if (!r) cap = ncap;
        return r;
    }
    NodeArrays arrays(const DevBuf& tbits) const {
        NodeArrays a;
        a.root = (int32_t*)R->n_root.p;
        a.parent = (int32_t*)R->n_parent.p;
        a.nseg = (int32_t*)R->n_nseg.p;
        a.status = (int32_t*)R->n_status.p;
        a.li = (int32_t*)R->n_li.p;
        a.hit_det = (int32_t*)R->n_hitdet.p;
        a.key = (unsigned long long*)R->n_key.p;
        a.lambda = (double*)R->n_lambda.p;
        a.hit = (double*)R->n_hit.p;
        a.aux = (double*)R->n_aux.p;
        a.cap = cap;
        a.hit_sub = nsub;
        a.old = (int32_t*)R->n_old.p;
        a.tbits = (unsigned long long*)tbits.p;
        return a;
    }
};

// Chunk arena: bump allocation out of large blocks (R->arena).  keep_log == false (record_segments = 0): the log is not kept — every
// chunk gets its own pool block and goes back to the pool as soon as its level is done (drop), so a solve holds two levels instead of
// all of them (beams, detector hits and counts are kept as always).
struct ChunkArena {
    std::vector<std::unique_ptr<DevBuf>>& blocks;
    size_t nd_bytes, rec_bytes;  // bytes of a record's double planes / of all its planes
    size_t block_bytes;
    bool keep_log;
    size_t top = 0;  // offset in the last block
    struct Mark {
        size_t blocks, top;
    };
    int alloc(int64_t cap, Chunk& c) {
        cap = std::max<int64_t>(cap, 1);
        const size_t cap_al = ((size_t)cap + 1) & ~(size_t)1;  // keep int planes 8-byte aligned
        const size_t need = cap_al * rec_bytes;
        if (!keep_log || blocks.empty() || top + need > blocks.back()->bytes) {
            auto b = std::make_unique<DevBuf>();
            if (int r = b->alloc(keep_log ? std::max(block_bytes, need) : need)) return r;
            blocks.push_back(std::move(b));
            top = 0;
        }
        char* base = static_cast<char*>(blocks.back()->p) + top;
        c.d = reinterpret_cast<double*>(base);
        c.i = reinterpret_cast<int32_t*>(base + cap_al * nd_bytes);
        c.cap = (int64_t)cap_al;
        c.count = 0;
        top += need;
        return BMO_OK;
    }
    void drop(const Chunk& c) {  // record_segments = 0 only; called behind the synchronisation of the chunk's launch
        PoolHold::Now at_once;
        for (size_t q = 0; q < blocks.size(); ++q)
            if (blocks[q]->p == (void*)c.d) {
                blocks.erase(blocks.begin() + (long)q);
                return;
            }
    }
    Mark mark() const { return Mark{blocks.size(), top}; }
    // everything allocated behind `m` goes back (allocation is a bump); the launch that could touch it has completed
    void rewind(const Mark& m) {
        PoolHold::Now at_once;
        while (blocks.size() > m.blocks) blocks.pop_back();
        top = m.top;
    }
};

// ---- step-kernel selection
using StepKernel = void (*)(StepParams);
struct StepKernels {
    StepKernel plain = nullptr, inw = nullptr;            // inw: the Beam kernels' variant with in-loop beam splitters (step_kernel_gauss handles them itself)
    StepKernel plain_wide = nullptr, inw_wide = nullptr;  // the 4-waves-per-SIMD builds of the two, for large launches (step_waves)
};
// + block_alloc scratch + per-lane columns: child cache (BMO_CC_MAX doubles) and the lane memory of tracing_step (BMO_LANE_MEM doubles).
// The scene tables stay in global memory: the kernels read them with scalar loads through constant-address-space pointers
// (bmo_lane.hpp "scalar scene access"); LDS holds the per-lane columns only.
constexpr size_t STEP_LDS_BYTES = 64 + (size_t)(BMO_CC_MAX + BMO_LANE_MEM) * BMO_BLOCK * 8;
static_assert(STEP_LDS_BYTES <= 48 * 1024, "the step kernels' dynamic LDS must fit the 48 KiB a launch gets without asking for more");

// The kernels of one (beam kind, extended-shapes level, fresh / retrace, sweep) combination — every instantiation of the step kernels is named here.
template <int KIND, int EXT, bool RETR, bool SWEEP>
StepKernels step_kernels_of() {
    StepKernels k;
    if constexpr (KIND == BMO_BEAM_GAUSSIAN) {
        k.plain = &step_kernel_gauss<EXT, RETR, SWEEP>;
    } else {
        constexpr int W = step_waves<KIND, EXT, RETR>();
        k.plain = &step_kernel<KIND, EXT, RETR, false, W, SWEEP>;
        k.inw = &step_kernel<KIND, EXT, RETR, true, W, SWEEP>;
#if !defined(BMO_MIN_WAVES)
        if constexpr (KIND == BMO_BEAM_RAY && EXT == 0 && !RETR && !SWEEP) {
            k.plain_wide = &step_kernel<BMO_BEAM_RAY, 0, false, false, 4>;
            k.inw_wide = &step_kernel<BMO_BEAM_RAY, 0, false, true, 4>;
        }
#endif
    }
    return k;
}
// the run-time level 0 … 3 as a template argument: f(std::integral_constant<int, ext>)
template <class F>
void with_ext(int ext, F&& f) {
    if (ext == 3) f(std::integral_constant<int, 3>{});
    else if (ext == 2) f(std::integral_constant<int, 2>{});
    else if (ext == 1) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}
#if defined(BMO_DEV_RAY_LDS_ONLY) || defined(BMO_DEV_GAUSS_ONLY)
// The developer builds refuse sweeps, yet have always carried the four SWEEP builds of step_kernel_gauss (a function that is no template
// names them).  Kept so: a developer build compares function by function with an earlier one (same set of kernels).
inline StepKernels dev_build_gauss_sweep_kernels(int ext) {
    StepKernels k;
    with_ext(ext, [&](auto e) { k = step_kernels_of<BMO_BEAM_GAUSSIAN, decltype(e)::value, false, true>(); });
    return k;
}
#endif
// ext: extended-shapes level of the kernels (bmo_lane.hpp sdf_leaf); a scene with a mesh BVH runs level 3 (level 2 + the BVH traversal).
// Sweeps (fresh solves, every level) have SWEEP builds of their own and no wide ones.
template <int KIND>
int select_step_kernels(int ext, bool retrace, bool sweep, StepKernels& k) {
    k = StepKernels{};
#if defined(BMO_DEV_RAY_LDS_ONLY)  // developer build (kernel work on one variant): everything else is refused, nothing falls back
    if constexpr (KIND == BMO_BEAM_RAY) {
        if (!retrace && ext == 0) k = step_kernels_of<BMO_BEAM_RAY, 0, false, false>();
    }
    if (!k.plain) return fail(BMO_ERR_UNSUPPORTED, "developer build: only step_kernel<RAY> is compiled in");
#elif defined(BMO_DEV_GAUSS_ONLY)  // developer build: the fresh GaussianBeamlet kernel of the plain-shapes level only
    if constexpr (KIND == BMO_BEAM_GAUSSIAN) {
        if (!retrace && ext == 0) k = step_kernels_of<BMO_BEAM_GAUSSIAN, 0, false, false>();
    }
    if (!k.plain) return fail(BMO_ERR_UNSUPPORTED, "developer build: only step_kernel_gauss<0, false> is compiled in");
#endif
    if (sweep && retrace) return fail(BMO_ERR_UNSUPPORTED, "sweeps are fresh solves");
#if defined(BMO_DEV_RAY_LDS_ONLY) || defined(BMO_DEV_GAUSS_ONLY)
    if (sweep) return fail(BMO_ERR_UNSUPPORTED, "developer build: no sweep kernels");
#else
    with_ext(ext, [&](auto e) {
        constexpr int E = decltype(e)::value;
        k = sweep ? step_kernels_of<KIND, E, false, true>() : (retrace ? step_kernels_of<KIND, E, true, false>() : step_kernels_of<KIND, E, false, false>());
    });
#endif
    return BMO_OK;
}

// Slot s of the first chunk holds root ray perm[s] (perm == nullptr: ray s); `slot_planes` are the batch's planes in slot order (the
// batch itself when perm == nullptr, its binned copy otherwise), so every read and write here is coalesced.  Beam nodes keep the
// bundle's numbering (root i is node i): everything downstream — result order, detector order, retrace — is independent of where a
// ray sits in the chunk.  Thread i fills slot i of the chunk and node i of the node table.
template <int KIND>
__global__ void init_roots_kernel(const double* __restrict__ planes, const double* __restrict__ slot_planes, const int32_t* __restrict__ lambda_idx,
                                  const int32_t* __restrict__ perm, int64_t n, Chunk c0, NodeArrays nodes, int32_t r_max, int32_t n_planes) {
    using L = Layout<KIND>;
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t cap = c0.cap;
    const double* Q = slot_planes;
    const bool cont = KIND == BMO_BEAM_GAUSSIAN && n_planes >= BMO_PLANES_GAUSSIAN_CONTINUED;
    if (KIND == BMO_BEAM_GAUSSIAN) {
        for (int b = 0; b < 3; ++b) {
            for (int p = 0; p < 6; ++p) c0.d[(LG::RAY_STRIDE * b + p) * cap + j] = Q[(6 * b + p) * n + j];
            c0.d[(LG::RAY_STRIDE * b + 6) * cap + j] = Q[19 * n + j];
        }
        // accumulated lengths: zero for a fresh beamlet; a batch that continues solved beamlets brings them along (include/bmo.h)
        c0.d[LG::LEN_A * cap + j] = cont ? Q[25 * n + j] : 0.0;
        c0.d[LG::LEN_B * cap + j] = cont ? Q[26 * n + j] : 0.0;
        c0.d[LG::OPL_C * cap + j] = cont ? Q[28 * n + j] : 0.0;
        c0.d[LG::OPL_W * cap + j] = cont ? Q[29 * n + j] : 0.0;
        c0.d[LG::OPL_D * cap + j] = cont ? Q[30 * n + j] : 0.0;
    } else {
        for (int p = 0; p < 6; ++p) c0.d[p * cap + j] = Q[p * n + j];
        c0.d[6 * cap + j] = Q[7 * n + j];
        if (KIND == BMO_BEAM_POLARIZED)
            for (int p = 0; p < 6; ++p) c0.d[(11 + p) * cap + j] = Q[(8 + p) * n + j];
        c0.d[L::OPL * cap + j] = 0.0;
    }
    c0.i[I_NODE * cap + j] = perm ? perm[j] : (int32_t)j;
    c0.i[I_K * cap + j] = 0;
    c0.i[I_HOBJ * cap + j] = -1;
    c0.i[I_HSHAPE * cap + j] = -1;
    c0.i[I_FLAGS * cap + j] = (1 < r_max) ? 0 : F_DEAD;
    // node j = root ray j of the bundle
    if (KIND == BMO_BEAM_GAUSSIAN) {
        nodes.aux[j * 4 + 0] = cont ? planes[27 * n + j] : 0.0;  // l0
        nodes.aux[j * 4 + 1] = planes[20 * n + j];
        nodes.aux[j * 4 + 2] = planes[21 * n + j];
        nodes.aux[j * 4 + 3] = planes[22 * n + j];
    }
    nodes.root[j] = (int32_t)j;
    nodes.parent[j] = -1;
    nodes.nseg[j] = 1;
    nodes.status[j] = 0;
    nodes.li[j] = lambda_idx[j];
    nodes.lambda[j] = planes[(KIND == BMO_BEAM_GAUSSIAN ? 18 : 6) * n + j];
    nodes.hit_det[j] = -1;
    nodes.key[j] = 0;
    if (nodes.tbits) nodes.tbits[j] = 1ull;  // the root itself: heap index 0
}

// What the driver needs of a beam kind: two plane counts, the sub-beams per node, and the kernels.
struct KindInfo {
    int kind, nd, abi_planes, nsub;
    bool gauss;
    void (*init_roots)(const double*, const double*, const int32_t*, const int32_t*, int64_t, Chunk, NodeArrays, int32_t, int32_t);
    int (*select)(int ext, bool retrace, bool sweep, StepKernels& k);
};
template <int KIND>
KindInfo kind_info() {
    return KindInfo{KIND, Layout<KIND>::ND, Layout<KIND>::ABI, KIND == BMO_BEAM_GAUSSIAN ? 3 : 1, KIND == BMO_BEAM_GAUSSIAN, &init_roots_kernel<KIND>,
                    &select_step_kernels<KIND>};
}

// ---- one launch of the step loop
struct LaunchPlan {
    int lane_shift;       // records per wave = 2^lane_shift (StepParams::lane_shift)
    int n_fuse;           // bounce levels fused into the launch (the in-place levels that fit may lower it: run_trace)
    int64_t sweep_lanes;  // lanes of a sweep launch's map, 0 otherwise
    int64_t n_waves;
    unsigned n_blocks;
    int64_t inwave_cap;  // StepParams::inwave_cap
    bool keep_kids;      // StepParams::pend / ::gkeep
};
// m: records of the launch.  Pure host arithmetic.
LaunchPlan plan_launch(int64_t m, int fuse_max, bool keep_log, size_t rec_bytes, bool has_split, bool inloop_splits, int32_t n_configs) {
    LaunchPlan p;
    const bool sweep = n_configs > 0;
    // records per wave (StepParams::lane_shift).  BMO_THIN_WAVES=<n>: a launch with fewer than n waves spreads its records over more waves.
    // Off by default: it took 6 % off the vignetted bundle while launches were level-synchronous, nothing since the beam splitters are
    // handled in the loop, and it costs small batches dearly (100 rays through config 2: 0.84 ms against 0.55 — every wave on a CU of
    // its own pays that CU's instruction- and scalar-cache warm-up): profiles/r03_ab_inwave.txt.
    p.lane_shift = 6;
    if (!sweep)
        while (p.lane_shift > 0 && ((m + (1ll << (p.lane_shift - 1)) - 1) >> (p.lane_shift - 1)) <= knobs().thin_waves) p.lane_shift -= 1;
    // Beam kernels: every launch fuses all its levels, whatever share of its beams ends, and handles its beam splitters in the loop
    // (step_kernel<.., INW>): holes cost lane time, launches cost the wait for the slowest march of every generation, and the second
    // is the dearer one — the vignetted bundle takes 2 launches and 14 ms this way, 12 launches and 23 ms when a launch fused fewer
    // levels the more of the previous launch's beams had ended (round 2; profiles/r03_ab_inwave.txt items 0 and 5).
    p.n_fuse = fuse_max;
    // the in-place levels of a launch are allocated up front: at most 24 GB of them (2^24 beams: 8 levels)
    if (keep_log) p.n_fuse = (int)std::min<int64_t>(p.n_fuse, 1 + (int64_t)(((size_t)24 << 30) / ((size_t)std::max<int64_t>(m, 1) * rec_bytes)));
    // a sweep launch: every configuration's run of slots padded to whole waves (at most 63 idle lanes per configuration present)
    p.sweep_lanes = sweep ? ((m + 63 * std::min<int64_t>(n_configs, m) + 63) & ~(int64_t)63) : 0;
    p.n_waves = sweep ? p.sweep_lanes >> 6 : (m + (1ll << p.lane_shift) - 1) >> p.lane_shift;
    p.n_blocks = (unsigned)((p.n_waves + BMO_BLOCK / 64 - 1) / (BMO_BLOCK / 64));
    // in-loop beam splitters: room for up to m reflected children more in the next launch's chunk (StepParams::inwave_cap)
    p.inwave_cap = (has_split && inloop_splits && p.n_fuse > 1) ? m : 0;
    // (kept reflected children, StepParams::pend: a lane can end its wave's loop with a kept child AND two fresh ones — one record more per lane)
    p.keep_kids = p.inwave_cap > 0 && knobs().keep_kids;
    return p;
}

// Buffers that serve every launch of a solve, grown when a launch has more records than any before it (the previous launch has completed
// by then: the old block goes back to the pool at once).
struct LaunchBufs {
    DevBuf gstage, gkeep;  // StepParams::gstage / ::gkeep (GaussianBeamlet: staging planes of the reflected children's rays, kept children)
    int64_t gstage_cap = 0;
    DevBuf pend;  // StepParams::pend (Beam kernels)
    int64_t pend_cap = 0;
    int fit(const KindInfo& K, const LaunchPlan& plan, int64_t m, size_t rec_bytes) {
        int rc;
        PoolHold::Now at_once;
        if (plan.keep_kids && !K.gauss && m > pend_cap) {
            pend.release();
            pend_cap = (m + 1) & ~(int64_t)1;
            if ((rc = pend.alloc((size_t)pend_cap * rec_bytes))) return rc;
        }
        if (K.gauss && m > gstage_cap) {
            gstage.release();
            gkeep.release();
            gstage_cap = ((m + m / 8 + 1) & ~(int64_t)1);
            if ((rc = gstage.alloc((size_t)gstage_cap * LG::STAGE_PLANES * 8)) || (rc = gkeep.alloc((size_t)gstage_cap * LG::KEEP_PLANES * 8))) return rc;
        }
        return BMO_OK;
    }
};

// The chunks of one launch: its input, the next launch's chunk and the in-place levels.
struct LaunchChunks {
    Chunk cur, nxt, inner[MAX_FUSE - 1];
    int n_inner = 0;  // in-place levels handed to the kernel (n_fuse - 1; the GaussianBeamlet kernels get one more: step_kernel_gauss)
    uint8_t* wl = nullptr;
};

void fill_step_params(StepParams& P, const KindInfo& K, const bmo_scene* scene, const char* dblob, const bmo_trace_opts* opts, const LaunchChunks& C,
                      const LaunchPlan& plan, const LaunchBufs& bufs, const NodeArrays& nodes, const OldSolution& old_tab, Counters* d_ctr, void* call_shards,
                      int step, int64_t n_nodes) {
    P.gstage = (double*)bufs.gstage.p;
    P.gstage_cap = bufs.gstage_cap;
    P.hdr = scene->hdr;
    P.blob = dblob;
    P.blob_bytes = (uint32_t)scene->blob.size();
    P.use_lds = 0;
    P.cur = C.cur;
    P.nxt = C.nxt;
    for (int q = 0; q < MAX_FUSE - 1; ++q) P.inner[q] = q < C.n_inner ? C.inner[q] : Chunk{nullptr, nullptr, 0, 0};
    P.n_fuse = plan.n_fuse;
    P.ctr = d_ctr;
    P.call_shards = static_cast<unsigned long long*>(call_shards);
    P.nodes = nodes;
    P.r_max = opts->r_max;
    P.parity = step & 1;
    P.old = old_tab;
    P.wave_last = C.wl;
    P.lane_shift = plan.lane_shift;
    P.inwave_cap = plan.inwave_cap;
    P.nodes0 = n_nodes;
    P.pend = Chunk{nullptr, nullptr, 0, 0};
    P.gkeep = (K.gauss && plan.keep_kids) ? (double*)bufs.gkeep.p : nullptr;
    if (plan.keep_kids && !K.gauss) {
        P.pend.d = static_cast<double*>(bufs.pend.p);
        P.pend.i = reinterpret_cast<int32_t*>(static_cast<char*>(bufs.pend.p) + (size_t)bufs.pend_cap * (size_t)K.nd * 8);
        P.pend.cap = bufs.pend_cap;
        P.pend.count = C.cur.count;
    }
    P.tile_order = nullptr;
    P.tile_cost = nullptr;
    // without feedback (StepParams::tile_order) a launch starts from the END of its chunk: a disc source has its marginal rays there,
    // children and survivors are queued in the order their parents got there — the slow ones last (StepParams::reverse)
    P.reverse = knobs().reverse >= 0 ? knobs().reverse : 1;
#if defined(BMO_DEV_TIMELINE)
    P.tl = nullptr;
#endif
}

// a[j] = j: tile ids here, node ids in order_nodes and run_trace, record numbers in bmo_result_view.inc.hpp
__global__ void iota_kernel(int32_t* a, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) a[j] = (int32_t)j;
}

// Longest-processing-time-first (StepParams::tile_order / ::tile_cost) for the first launch of a solve: the batch keeps the time every tile
// took, the next solve of the batch sorts its tiles by it.  A retrace with a freshly uploaded batch starts from the retraced solution's times.
int tile_order_feedback(StepParams& P, bmo_device_batch* batch, const bmo_trace_result* prev, unsigned n_blocks, hipStream_t stream) {
    int rc;
    if (batch->tile_n != (int64_t)n_blocks) {
        PoolHold::Now at_once;
        batch->cost_valid = false;
        batch->tile_n = 0;
        batch->tile_cost.release(), batch->tile_order.release(), batch->lpt_ids.release(), batch->lpt_keys.release(), batch->lpt_tmp.release();
        if ((rc = batch->tile_cost.alloc((size_t)n_blocks * 4)) || (rc = batch->tile_order.alloc((size_t)n_blocks * 4)) ||
            (rc = batch->lpt_ids.alloc((size_t)n_blocks * 4)) || (rc = batch->lpt_keys.alloc((size_t)n_blocks * 4)))
            return rc;
        hipLaunchKernelGGL(iota_kernel, dim3((n_blocks + 255) / 256), dim3(256), 0, stream, (int32_t*)batch->lpt_ids.p, (int64_t)n_blocks);
        batch->tile_n = (int64_t)n_blocks;
    }
    if (!batch->cost_valid && prev && prev->tile_n == (int64_t)n_blocks && prev->tile_cost.p) {  // feedback from the solution that is retraced
        HIP_TRY(hipMemcpyAsync(batch->tile_cost.p, prev->tile_cost.p, (size_t)n_blocks * 4, hipMemcpyDeviceToDevice, stream));
        batch->cost_valid = true;
    }
    if (batch->cost_valid) {
        // (the sort's temporary lives in the batch across solves: the first sort over these tiles makes it)
        CUB_TRY(scratch_in(batch->lpt_tmp), hipcub::DeviceRadixSort::SortPairsDescending(cub_tmp, cub_bytes, (const uint32_t*)batch->tile_cost.p, (uint32_t*)batch->lpt_keys.p,
                                                                                         (const int32_t*)batch->lpt_ids.p, (int32_t*)batch->tile_order.p, (int)n_blocks, 0, 32, stream));
        P.tile_order = (const int32_t*)batch->tile_order.p;
    }
    DBG("step 0 tile order: %s", P.tile_order ? "by the cost of the batch's previous solve" : "as laid out (no costs yet)");
    P.tile_cost = (uint32_t*)batch->tile_cost.p;
    batch->cost_valid = true;  // (after this launch)
    return BMO_OK;
}

// ---- lane map of a sweep launch (StepParams::sweep): key = configuration of every slot of the launch's chunk (node -> root -> root_cfg),
// a stable sort by it, the runs padded to whole waves.  beg / end: first and one-past-last sorted position of every configuration.
__global__ void sweep_key_kernel(Chunk c, const int32_t* __restrict__ root, const int32_t* __restrict__ root_cfg, int64_t m, uint32_t* __restrict__ key,
                                 int32_t* __restrict__ slot) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    key[j] = (uint32_t)root_cfg[root[c.i[I_NODE * c.cap + j]]];
    slot[j] = (int32_t)j;
}
__global__ void sweep_bounds_kernel(const uint32_t* __restrict__ key, int64_t m, int32_t* __restrict__ beg, int32_t* __restrict__ end) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t k = key[i];
    if (i == 0 || key[i - 1] != k) beg[k] = (int32_t)i;
    if (i == m - 1 || key[i + 1] != k) end[k] = (int32_t)(i + 1);
}
__global__ void sweep_pad_kernel(const int32_t* __restrict__ beg, const int32_t* __restrict__ end, int32_t n_configs, int32_t* __restrict__ padded) {
    const int32_t c = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= n_configs) return;
    padded[c] = (end[c] - beg[c] + 63) & ~63;
}
__global__ void sweep_scatter_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ slot, int64_t m, const int32_t* __restrict__ beg,
                                     const int32_t* __restrict__ pstart, int64_t lanes, int32_t* __restrict__ map, unsigned long long* __restrict__ overflow) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t k = key[i];
    const int64_t v = (int64_t)pstart[k] + (i - beg[k]);
    if (v < lanes) map[v] = slot[i];
    else atomicAdd(overflow, 1ull);
}
// Sweep lane map (StepParams::sweep) of a launch over the m records of `cur`: key = configuration of every slot, stable sort (slot order
// within a configuration), runs padded to whole waves.
int build_sweep_lane_map(const bmo_trace_result* R, const Chunk& cur, int64_t sweep_lanes, Counters* d_ctr, hipStream_t stream, DevBuf& sw_map) {
    int rc;
    const int64_t m = cur.count;
    const int32_t K = R->n_configs;
    DevBuf key, key_s, slot, slot_s, beg, end, padded, pstart;
    Temps tmp;
    if ((rc = key.alloc((size_t)m * 4)) || (rc = key_s.alloc((size_t)m * 4)) || (rc = slot.alloc((size_t)m * 4)) || (rc = slot_s.alloc((size_t)m * 4)) ||
        (rc = beg.alloc((size_t)K * 4)) || (rc = end.alloc((size_t)K * 4)) || (rc = padded.alloc((size_t)K * 4)) || (rc = pstart.alloc((size_t)K * 4)) ||
        (rc = sw_map.alloc((size_t)sweep_lanes * 4)))
        return rc;
    int kbits = 1;
    while (kbits < 32 && ((uint32_t)(K - 1) >> kbits)) ++kbits;
    const unsigned mb = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(sweep_key_kernel, dim3(mb), dim3(256), 0, stream, cur, (const int32_t*)R->n_root.p, (const int32_t*)R->d_root_cfg.p, m,
                       (uint32_t*)key.p, (int32_t*)slot.p);
    CUB_TRY(tmp, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const uint32_t*)key.p, (uint32_t*)key_s.p, (const int32_t*)slot.p, (int32_t*)slot_s.p, (int)m, 0, kbits, stream));
    HIP_TRY(hipMemsetAsync(beg.p, 0, (size_t)K * 4, stream));
    HIP_TRY(hipMemsetAsync(end.p, 0, (size_t)K * 4, stream));
    hipLaunchKernelGGL(sweep_bounds_kernel, dim3(mb), dim3(256), 0, stream, (const uint32_t*)key_s.p, m, (int32_t*)beg.p, (int32_t*)end.p);
    hipLaunchKernelGGL(sweep_pad_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, stream, (const int32_t*)beg.p, (const int32_t*)end.p, K, (int32_t*)padded.p);
    CUB_TRY(tmp, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)padded.p, (int32_t*)pstart.p, (int)K, stream));
    HIP_TRY(hipMemsetAsync(sw_map.p, 0xFF, (size_t)sweep_lanes * 4, stream));
    hipLaunchKernelGGL(sweep_scatter_kernel, dim3(mb), dim3(256), 0, stream, (const uint32_t*)key_s.p, (const int32_t*)slot_s.p, m, (const int32_t*)beg.p,
                       (const int32_t*)pstart.p, sweep_lanes, (int32_t*)sw_map.p, &d_ctr->overflow);
    HIP_TRY(hipGetLastError());
    return BMO_OK;
}

#if defined(BMO_DEV_TIMELINE)  // developer builds, BMO_TIMELINE=1: how many waves are at work over the course of every launch
int print_timeline(const unsigned long long* tl, size_t nw, int steps) {
    std::vector<unsigned long long> t(2 * nw + 3);
    HIP_TRY(hipMemcpy(t.data(), tl, nw * 16 + 24, hipMemcpyDeviceToHost));
    {
        const double a = (double)t[2 * nw], b2 = (double)t[2 * nw + 1], c2 = (double)t[2 * nw + 2], sum = a + b2 + c2;
        // (finer timers inside the lane code — per sdf_any / normal_any / object — measure mostly their own s_memrealtime latency)
        fprintf(stderr, "[bmo] timeline step %d: wave time before / in / after tracing_step: %.1f %% / %.1f %% / %.1f %%  (%.1f us per wave in all)\n", steps,
                100 * a / sum, 100 * b2 / sum, 100 * c2 / sum, sum / nw / 100.0);
    }
    unsigned long long t0 = ~0ull, t1 = 0;
    for (size_t w = 0; w < nw; ++w) {
        t0 = std::min(t0, t[2 * w]);
        t1 = std::max(t1, t[2 * w + 1]);
    }
    const double span = (double)(t1 - t0);
    const int NB = 40;
    std::vector<double> busy(NB, 0.0);  // wave residency integrated per bin
    for (size_t w = 0; w < nw; ++w) {
        const double a = (double)(t[2 * w] - t0) / span * NB, b2 = (double)(t[2 * w + 1] - t0) / span * NB;
        for (int q = (int)a; q < NB && q <= (int)b2; ++q) busy[q] += std::min(b2, (double)q + 1) - std::max(a, (double)q);
    }
    fprintf(stderr, "[bmo] timeline step %d: %zu waves, span %.3f ms; mean waves at work per 1/%d of the span:\n ", steps, nw, span / 1e5, NB);
    for (int q = 0; q < NB; ++q) fprintf(stderr, " %.0f", busy[q]);
    fprintf(stderr, "\n");
    {  // the waves that end last: where in the grid they sit, when they started
        std::vector<size_t> idx(nw);
        for (size_t w = 0; w < nw; ++w) idx[w] = w;
        const size_t top = std::min<size_t>(nw, 12);
        std::partial_sort(idx.begin(), idx.begin() + (long)top, idx.end(), [&](size_t a, size_t b2) { return t[2 * a + 1] > t[2 * b2 + 1]; });
        fprintf(stderr, "[bmo] timeline step %d: last waves to end (wave of the grid: start .. end in ms):", steps);
        for (size_t q = 0; q < top; ++q) fprintf(stderr, "  %zu: %.3f .. %.3f", idx[q], (double)(t[2 * idx[q]] - t0) / 1e5, (double)(t[2 * idx[q] + 1] - t0) / 1e5);
        fprintf(stderr, "\n");
        std::vector<double> dur(nw);
        for (size_t w = 0; w < nw; ++w) dur[w] = (double)(t[2 * w + 1] - t[2 * w]) / 1e5;
        std::vector<double> srt = dur;
        std::sort(srt.begin(), srt.end());
        fprintf(stderr, "[bmo] timeline step %d: wave durations ms p50 %.3f p90 %.3f p99 %.3f p99.9 %.3f max %.3f\n", steps, srt[nw / 2], srt[nw * 9 / 10], srt[nw * 99 / 100],
                srt[std::min(nw - 1, nw * 999 / 1000)], srt[nw - 1]);
    }
    return BMO_OK;
}
#endif

// Queues the launch between its two timing events (one pair per step out of the context's pool, read after the loop: nothing but the counter
// read-back sits between two launches), reads the counters back and waits.
int launch_step(DevCtx& ctx, const StepKernels& kern, const LaunchPlan& plan, const StepParams& P, int step, Counters* d_ctr, int64_t wide_min_waves) {
    hipStream_t stream = ctx.stream;
    while ((int)ctx.step_ev.size() < 2 * (step + 1)) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ctx.step_ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ctx.step_ev[2 * step], stream));
    // (the 4-waves-per-SIMD build for a launch that fills the device at that occupancy — 256 CUs x 16 waves —, the 3-waves one below: step_waves.
    //  Between 4 096 and ~10 000 waves the two scenes measured disagree — config 5 - 13 % / - 6 %, config 2 + 2 % / + 3 % — and the larger effect decides.)
    const bool wide = kern.plain_wide && plan.n_waves >= wide_min_waves;
    const StepKernel k = (plan.inwave_cap > 0 && kern.inw) ? (wide ? kern.inw_wide : kern.inw) : (wide ? kern.plain_wide : kern.plain);
    if (!k) return fail(BMO_ERR_INTERNAL, "no step kernel selected for this beam kind / scene level");
    DBG("step %d kernel build: %s, %s", step, wide ? "4 waves per SIMD" : "default waves per SIMD", (plan.inwave_cap > 0 && kern.inw) ? "in-loop splitters" : "splits end the loop");
    hipLaunchKernelGGL(k, dim3(plan.n_blocks), dim3(BMO_BLOCK), STEP_LDS_BYTES, stream, P);
    HIP_TRY(hipEventRecord(ctx.step_ev[2 * step + 1], stream));
    HIP_TRY(hipMemcpyAsync(ctx.pinned, d_ctr, sizeof(Counters), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    return BMO_OK;
}

// (root, depth, path) keys packed into as few bits as this solve needs: the radix sort of the final ordering runs 3-4 passes over
// 32-bit keys instead of 8 over 64-bit ones.  Trees of up to MAX_PATH_LEVELS levels.
constexpr int MAX_PATH_LEVELS = 26;
__global__ void pack_keys_kernel(const int32_t* __restrict__ root_of, const unsigned long long* __restrict__ key, int64_t n, int bits_depth, int bits_path,
                                 uint32_t* __restrict__ k32, unsigned long long* __restrict__ k64) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = key[i];
    const unsigned long long root = (unsigned long long)root_of[i], depth = k >> 32, path = k & ((1ull << bits_path) - 1ull);
    const unsigned long long packed = (root << (bits_depth + bits_path)) | (depth << bits_path) | path;
    if (k32) k32[i] = (uint32_t)packed;
    else k64[i] = packed;
}
// ---- ordering of shallow trees (up to MAX_HEAP_LEVELS levels below the root: what one to five splitters in a row give) without a
// sort: node (depth, path) sits at index 2^depth - 1 + path of its root's tree laid out as a heap, and heap order IS (depth, path)
// order.  Every root collects the heap indices of its nodes in one 64-bit word; a node's position in the canonical order is then
// (number of nodes of the roots before its own: one scan over the roots) + (number of set bits below its own).
constexpr int MAX_HEAP_LEVELS = 5;
__device__ __forceinline__ unsigned heap_index(unsigned long long key) {
    const unsigned depth = (unsigned)(key >> 32);
    return (1u << depth) - 1u + (unsigned)(key & ((1ull << depth) - 1ull));
}
__global__ void tree_bits_kernel(const int32_t* __restrict__ root_of, const unsigned long long* __restrict__ key, int64_t n, unsigned long long* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    atomicOr(&bits[root_of[i]], 1ull << heap_index(key[i]));
}
__global__ void tree_count_kernel(const unsigned long long* __restrict__ bits, int64_t n_roots, int32_t* __restrict__ cnt) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_roots) cnt[r] = __popcll(bits[r]);
}
__global__ void tree_rank_kernel(const int32_t* __restrict__ root_of, const unsigned long long* __restrict__ key, int64_t n, const unsigned long long* __restrict__ bits,
                                 const int32_t* __restrict__ base, int32_t* __restrict__ order) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t r = root_of[i];
    const unsigned h = heap_index(key[i]);
    order[base[r] + __popcll(bits[r] & ((1ull << h) - 1ull))] = (int32_t)i;
}
// ---- ordering of beam trees deeper than MAX_PATH_LEVELS (cavities: a splitter facing a mirror): the path no longer fits a key, so
// the rank of every node within its tree level is built level by level from its parent's rank (a splitting beam has exactly two
// children, transmitted first): rank(child) = 2 * #(splitting parents of smaller rank) + w.
__global__ void node_depth_kernel(const unsigned long long* __restrict__ key, int64_t n, uint32_t* __restrict__ depth) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) depth[i] = (uint32_t)(key[i] >> 32);
}
__global__ void level_starts_kernel(const uint32_t* __restrict__ sorted_depth, int64_t n, int64_t max_depth, int32_t* __restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t d = sorted_depth[i], dprev = i ? (int64_t)sorted_depth[i - 1] : -1;
    for (int64_t x = dprev + 1; x <= d; ++x) start[x] = (int32_t)i;
    if (i == n - 1)
        for (int64_t x = d + 1; x <= max_depth + 1; ++x) start[x] = (int32_t)n;
}
__global__ void level_root_rank_kernel(const int32_t* __restrict__ ids, int32_t cnt, int32_t* __restrict__ rank) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cnt) rank[ids[i]] = i;  // level 0: the roots, in node id = bundle order (the depth sort is stable)
}
__global__ void level_flag_kernel(const int32_t* __restrict__ ids, int32_t cnt, const int32_t* __restrict__ parent, const unsigned long long* __restrict__ key,
                                  const int32_t* __restrict__ rank, int32_t* __restrict__ flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const int32_t nd = ids[i];
    if (!(key[nd] & 1ull)) flag[rank[parent[nd]]] = 1;
}
__global__ void level_rank_kernel(const int32_t* __restrict__ ids, int32_t cnt, const int32_t* __restrict__ parent, const unsigned long long* __restrict__ key,
                                  const int32_t* __restrict__ scan, int32_t* __restrict__ rank) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const int32_t nd = ids[i];
    rank[nd] = 2 * scan[rank[parent[nd]]] + (int32_t)(key[nd] & 1ull);
}
__global__ void gather_u32_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ src, int64_t n, uint32_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (uint32_t)src[idx[i]];
}
__global__ void root_depth_key_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ root_of, const unsigned long long* __restrict__ key, int64_t n,
                                      int bits_depth, unsigned long long* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t nd = idx[i];
    out[i] = ((unsigned long long)root_of[nd] << bits_depth) | (key[nd] >> 32);
}
// ---- canonical node order (bundle order x BFS order): sort by (root, depth, path).  Three paths by the depth of the deepest tree;
// all leave the order in R->order, queued on the stream.
inline int bits_for(unsigned long long v) {  // bits needed to hold values 0..v
    int b = 0;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// trees of up to MAX_HEAP_LEVELS levels: the heap indices of every root's nodes as a bitmap (`tbits`: collected while the nodes were made)
int order_by_heap_index(bmo_trace_result* R, int64_t n, int64_t n_nodes, const DevBuf& tbits, hipStream_t stream, Temps& temps) {
    DevBuf *bits = temps.take((size_t)n * 8), *cnt = temps.take((size_t)n * 4), *base = temps.take((size_t)n * 4);
    if (!bits || !cnt || !base) return BMO_ERR_OOM;
    const unsigned nb = (unsigned)((n_nodes + 255) / 256), rb = (unsigned)((n + 255) / 256);
    const unsigned long long* b = (const unsigned long long*)(tbits.p ? tbits.p : bits->p);
    if (!tbits.p) {
        HIP_TRY(hipMemsetAsync(bits->p, 0, (size_t)n * 8, stream));
        hipLaunchKernelGGL(tree_bits_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)R->n_root.p, (const unsigned long long*)R->n_key.p, n_nodes,
                           (unsigned long long*)bits->p);
    }
    hipLaunchKernelGGL(tree_count_kernel, dim3(rb), dim3(256), 0, stream, b, n, (int32_t*)cnt->p);
    CUB_TRY(temps, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)cnt->p, (int32_t*)base->p, (int)n, stream));
    hipLaunchKernelGGL(tree_rank_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)R->n_root.p, (const unsigned long long*)R->n_key.p, n_nodes, b,
                       (const int32_t*)base->p, (int32_t*)R->order.p);
    return BMO_OK;
}

// up to MAX_PATH_LEVELS levels: one radix sort on packed (root, depth, path) keys, 32 bits wide where they fit.  R->order holds the iota.
int order_by_packed_keys(bmo_trace_result* R, int64_t n_nodes, int bits_root, int bits_depth, int bits_path, hipStream_t stream, Temps& temps) {
    const int bits = bits_root + bits_depth + bits_path;
    const bool narrow = bits <= 32;
    DevBuf *k_in = temps.take((size_t)n_nodes * (narrow ? 4 : 8)), *k_out = temps.take((size_t)n_nodes * (narrow ? 4 : 8)), *v_out = temps.take((size_t)n_nodes * 4);
    if (!k_in || !k_out || !v_out) return BMO_ERR_OOM;
    hipLaunchKernelGGL(pack_keys_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, stream, (const int32_t*)R->n_root.p, (const unsigned long long*)R->n_key.p,
                       n_nodes, bits_depth, bits_path, narrow ? (uint32_t*)k_in->p : nullptr, narrow ? nullptr : (unsigned long long*)k_in->p);
    if (narrow)
        CUB_TRY(temps, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const uint32_t*)k_in->p, (uint32_t*)k_out->p, (const int32_t*)R->order.p, (int32_t*)v_out->p,
                                                          (int)n_nodes, 0, bits, stream));
    else
        CUB_TRY(temps, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const unsigned long long*)k_in->p, (unsigned long long*)k_out->p, (const int32_t*)R->order.p,
                                                          (int32_t*)v_out->p, (int)n_nodes, 0, bits, stream));
    std::swap(R->order.p, v_out->p);  // the sorted ids are the order; the iota stays with the temporaries
    std::swap(R->order.bytes, v_out->bytes);
    return BMO_OK;
}

// deep trees: ranks within each tree level, level by level, then sort by (root, depth, rank).  R->order holds the iota.
// Synchronises in the middle (the level starts are read back) and at the end.
int order_level_by_level(bmo_trace_result* R, int64_t n_nodes, int64_t md, int bits_root, int bits_depth, hipStream_t stream) {
    int rc;
    const unsigned nb = (unsigned)((n_nodes + 255) / 256);
    const int32_t* parent = (const int32_t*)R->n_parent.p;
    const unsigned long long* key = (const unsigned long long*)R->n_key.p;
    DevBuf depth, depth_sorted, by_depth, starts, rank, flag, scan, k64, k64_out, ids2, keys_in, keys_out, vals_out;
    Temps tmp;  // one scratch block for the sorts and the per-level scans
    if ((rc = depth.alloc((size_t)n_nodes * 4)) || (rc = depth_sorted.alloc((size_t)n_nodes * 4)) || (rc = by_depth.alloc((size_t)n_nodes * 4)) ||
        (rc = starts.alloc((size_t)(md + 2) * 4)) || (rc = rank.alloc((size_t)n_nodes * 4)) || (rc = flag.alloc((size_t)n_nodes * 4)) ||
        (rc = scan.alloc((size_t)n_nodes * 4)) || (rc = k64.alloc((size_t)n_nodes * 8)) || (rc = k64_out.alloc((size_t)n_nodes * 8)) ||
        (rc = ids2.alloc((size_t)n_nodes * 4)) || (rc = vals_out.alloc((size_t)n_nodes * 4)) || (rc = keys_in.alloc((size_t)n_nodes * 4)) ||
        (rc = keys_out.alloc((size_t)n_nodes * 4)))
        return rc;
    hipLaunchKernelGGL(node_depth_kernel, dim3(nb), dim3(256), 0, stream, key, n_nodes, (uint32_t*)depth.p);
    CUB_TRY(tmp, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const uint32_t*)depth.p, (uint32_t*)depth_sorted.p, (const int32_t*)R->order.p, (int32_t*)by_depth.p,
                                                    (int)n_nodes, 0, bits_depth, stream));
    hipLaunchKernelGGL(level_starts_kernel, dim3(nb), dim3(256), 0, stream, (const uint32_t*)depth_sorted.p, n_nodes, md, (int32_t*)starts.p);
    std::vector<int32_t> h_start((size_t)md + 2);
    HIP_TRY(hipMemcpyAsync(h_start.data(), starts.p, (size_t)(md + 2) * 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const int32_t* ids = (const int32_t*)by_depth.p;
    hipLaunchKernelGGL(level_root_rank_kernel, dim3((unsigned)((h_start[1] + 255) / 256)), dim3(256), 0, stream, ids, h_start[1], (int32_t*)rank.p);
    int32_t max_level = h_start[1];
    for (int64_t d = 1; d <= md; ++d) {
        const int32_t cnt_prev = h_start[d] - h_start[d - 1], cnt = h_start[d + 1] - h_start[d];
        if (cnt <= 0 || cnt_prev <= 0) continue;
        max_level = std::max(max_level, cnt);
        const unsigned lb = (unsigned)((cnt + 255) / 256);
        HIP_TRY(hipMemsetAsync(flag.p, 0, (size_t)cnt_prev * 4, stream));
        hipLaunchKernelGGL(level_flag_kernel, dim3(lb), dim3(256), 0, stream, ids + h_start[d], cnt, parent, key, (const int32_t*)rank.p, (int32_t*)flag.p);
        CUB_TRY(tmp, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)flag.p, (int32_t*)scan.p, (int)cnt_prev, stream));
        hipLaunchKernelGGL(level_rank_kernel, dim3(lb), dim3(256), 0, stream, ids + h_start[d], cnt, parent, key, (const int32_t*)scan.p, (int32_t*)rank.p);
    }
    // LSD: by rank within the level, then (stable) by (root, depth)
    hipLaunchKernelGGL(gather_u32_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)R->order.p, (const int32_t*)rank.p, n_nodes, (uint32_t*)keys_in.p);
    CUB_TRY(tmp, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const uint32_t*)keys_in.p, (uint32_t*)keys_out.p, (const int32_t*)R->order.p, (int32_t*)ids2.p,
                                                    (int)n_nodes, 0, bits_for((unsigned long long)max_level), stream));
    hipLaunchKernelGGL(root_depth_key_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)ids2.p, (const int32_t*)R->n_root.p, key, n_nodes, bits_depth,
                       (unsigned long long*)k64.p);
    CUB_TRY(tmp, hipcub::DeviceRadixSort::SortPairs(cub_tmp, cub_bytes, (const unsigned long long*)k64.p, (unsigned long long*)k64_out.p, (const int32_t*)ids2.p,
                                                    (int32_t*)vals_out.p, (int)n_nodes, 0, bits_root + bits_depth, stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));  // the level tables go back to the pool
    std::swap(R->order.p, vals_out.p);
    std::swap(R->order.bytes, vals_out.bytes);
    return BMO_OK;
}

// max_depth: Counters::max_depth as read back after the last launch.  force_sort / force_deep (test hooks, SolveSwitches): the radix-sort /
// level-by-level path for any tree.  Says which path ran, once per solve.
int order_nodes(bmo_trace_result* R, int64_t n, int64_t n_nodes, unsigned long long max_depth, const DevBuf& tbits, bool force_sort, bool force_deep,
                hipStream_t stream, Temps& temps) {
    int rc;
    if ((rc = R->order.alloc((size_t)std::max<int64_t>(n_nodes, 1) * 4))) return rc;
    const bool roots_only = n_nodes <= n, heap = !roots_only && max_depth <= (unsigned long long)MAX_HEAP_LEVELS && !force_sort && !force_deep;
    const bool packed = max_depth <= (unsigned long long)MAX_PATH_LEVELS && !force_deep;
    DBG("node order: %s", roots_only ? "bundle order" : (heap ? "heap index" : (packed ? "packed keys" : "level by level")));
    if (heap) return order_by_heap_index(R, n, n_nodes, tbits, stream, temps);
    if (n_nodes > 0) hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, stream, (int32_t*)R->order.p, n_nodes);
    if (roots_only) return BMO_OK;
    const int bits_depth = bits_for(max_depth), bits_root = bits_for((unsigned long long)std::max<int64_t>(n - 1, 0));
    if (packed) return order_by_packed_keys(R, n_nodes, bits_root, bits_depth, (int)max_depth /* one bit per level */, stream, temps);
    return order_level_by_level(R, n_nodes, (int64_t)max_depth, bits_root, bits_depth, stream);
}

// ---- detector hits in reference push! order.  The hit table holds the rows of detector 0, then detector 1 ..., each in canonical node
// order, nsub rows per hit.  A workgroup takes 256 consecutive canonical nodes (a tile): hit_count_kernel counts every tile's rows per
// detector, one exclusive scan over the nd x n_tiles counts (detector-major) gives every tile its first row per detector, and
// hit_gather_kernel ranks a tile's hits among themselves.  Nothing here scales with nd x n_nodes.
//
// Ranks the lanes of a wave by detector: `rank` = lanes below this one with the same detector d (d < 0: no hit), and once per distinct
// detector of the wave (on the first lane that has it) f(detector, lanes with it).  As many trips as the wave has distinct detectors.
template <class F>
__device__ __forceinline__ int wave_rank_by_detector(int32_t d, F&& f) {
    const int lane = (int)(threadIdx.x & 63u);
    int rank = 0;
    unsigned long long todo = __ballot(d >= 0);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int32_t dd = __shfl(d, lead);
        const unsigned long long same = __ballot(d == dd);
        if (d == dd) rank = __popcll(same & ((1ull << lane) - 1ull));
        if (lane == lead) f(dd, __popcll(same));
        todo &= ~same;
    }
    return rank;
}
// cnt[d * n_tiles + tile] = rows of detector d in the tile (nsub per hit), cnt[n_det * n_tiles] = 0 (the scan leaves the total there);
// seg_shards[16 (tile & 63) + 1] += the segment counts of nodes [256 tile, 256 tile + 256): a sum of integers, in any order, one atomic
// per workgroup, spread over the 64 lines of the call-counter shards (12 000 workgroups adding to ONE word took 147 us per config-2
// solve, 12 ns per add: profiles/finish_pass_ab.txt).  n_det == 0 (no detectors): the segment count alone.
__global__ void __launch_bounds__(256) hit_count_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ hit_det, const int32_t* __restrict__ nseg, int64_t n,
                                                        int32_t n_det, int32_t nsub, int32_t* __restrict__ cnt, unsigned long long* __restrict__ seg_shards) {
    __shared__ int32_t s_cnt[MAX_DETECTORS + 1];
    __shared__ long long s_seg[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int q = threadIdx.x; q < n_det; q += 256) s_cnt[q] = 0;
    long long seg = i < n ? (long long)nseg[i] : 0;
    for (int o = 32; o > 0; o >>= 1) seg += __shfl_xor(seg, o);
    if ((threadIdx.x & 63u) == 0) s_seg[threadIdx.x >> 6] = seg;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&seg_shards[(blockIdx.x & 63u) * 16u + 1u], (unsigned long long)(s_seg[0] + s_seg[1] + s_seg[2] + s_seg[3]));
    if (n_det == 0) return;
    int32_t d = i < n ? hit_det[order[i]] : -1;
    if (d >= n_det) d = -1;
    wave_rank_by_detector(d, [&](int32_t dd, int lanes) { atomicAdd(&s_cnt[dd], lanes); });
    __syncthreads();
    for (int q = threadIdx.x; q < n_det; q += 256) cnt[(int64_t)q * gridDim.x + blockIdx.x] = s_cnt[q] * nsub;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[(int64_t)n_det * gridDim.x] = 0;
}

// A workgroup takes 256 consecutive canonical nodes: their (id, destination) pairs go to LDS once, then the 72-byte records are copied
// as contiguous runs, one double per thread and turn (the first form of this kernel re-read the three index tables for each of
// the 9 doubles: 152 us per C2 solve for 0.3 GB of traffic).
// A node's first row = its tile's first row for the node's detector (`offs`: the scanned counts of hit_count_kernel, n_det x
// n_tiles + 1 of them) + nsub x the tile's earlier hits on that detector, counted per wave in LDS; the first workgroup also leaves every
// detector's first row and the number of rows in det_off (TailBlock).
__global__ void __launch_bounds__(256) hit_gather_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ hit_det, const double* __restrict__ hit, int64_t n,
                                                         int32_t nsub, const int32_t* __restrict__ offs, int64_t cap, double* __restrict__ out,
                                                         int32_t* __restrict__ out_node, unsigned long long* __restrict__ overflow, int32_t n_det,
                                                         int32_t* __restrict__ det_off) {
    __shared__ int32_t s_nd[256], s_pos[256];
    __shared__ int32_t s_wave[4][MAX_DETECTORS + 1];  // hits of every wave of the tile on every detector
    const int64_t i0 = (int64_t)blockIdx.x * 256;
    {
        const int64_t i = i0 + threadIdx.x;
        int32_t nd = -1, pos = -1;
        if (blockIdx.x == 0)
            for (int q = threadIdx.x; q <= n_det; q += 256) det_off[q] = offs[(int64_t)q * gridDim.x];
        for (int q = threadIdx.x; q < 4 * n_det; q += 256) s_wave[q / n_det][q % n_det] = 0;
        __syncthreads();
        int32_t d = -1;
        if (i < n) {
            nd = order[i];
            d = hit_det[nd];
            if (d >= n_det) d = -1;
        }
        const int w = (int)(threadIdx.x >> 6);
        const int rank = wave_rank_by_detector(d, [&](int32_t dd, int lanes) { s_wave[w][dd] = lanes; });
        __syncthreads();
        if (d >= 0) {
            int before = rank;
            for (int q = 0; q < w; ++q) before += s_wave[q][d];
            pos = offs[(int64_t)d * gridDim.x + blockIdx.x] + before * nsub;
            if ((int64_t)pos + nsub > cap) {
                atomicAdd(overflow, 1ull);
                pos = -1;
            } else {
                for (int q = 0; q < nsub; ++q) out_node[pos + q] = (int32_t)i;
            }
        }
        s_nd[threadIdx.x] = nd;
        s_pos[threadIdx.x] = pos;
    }
    __syncthreads();
    const int width = 9 * nsub;
    // element t = e * width + k of the workgroup's 256 records; t advances by 256 per turn: (e, k) by (256 / width, 256 % width) with a
    // carry, no division per element
    const int de = 256 / width, dk = 256 % width;
    int e = (int)threadIdx.x / width, k = (int)threadIdx.x % width;
    for (int t = threadIdx.x; t < 256 * width; t += 256) {
        const int32_t pos = s_pos[e];
        if (pos >= 0) out[(int64_t)pos * 9 + k] = hit[(int64_t)s_nd[e] * width + k];
        e += de;
        k += dk;
        if (k >= width) {
            k -= width;
            e += 1;
        }
    }
}
// Segment count and detector tables of a solve, queued: the counts per tile, their scan, the gather.  d_tail->shards (word 1) and
// d_tail->det_off (the first row of every detector, the number of rows behind them) come back with the block's read-back.
int count_and_gather_hits(bmo_trace_result* R, int nsub, int64_t n, int64_t n_nodes, TailBlock* d_tail, hipStream_t stream, Temps& temps) {
    int rc;
    const int nd = R->n_detectors;  // (at most MAX_DETECTORS: run_trace refuses more before it sizes the tail block)
    const unsigned nb = (unsigned)((n_nodes + 255) / 256);
    const int64_t tot = (int64_t)nd * nb + 1;  // counts of every (detector, tile), detector-major, and one more for the total
    // the hit table is sized before the counts are back on the host: a beam with a hit has ended and every splitting beam has two
    // children, so there are at most (beams + roots) / 2 of them
    const int64_t bound = (n_nodes + n) / 2 * nsub + nsub;
    if (tot >= ((int64_t)1 << 31) || bound >= ((int64_t)1 << 31)) return fail(BMO_ERR_UNSUPPORTED, "detector rows exceed 2^31: split the batch");
    DevBuf *cnt = nullptr, *offs = nullptr;
    if (nd > 0 && (!(cnt = temps.take((size_t)tot * 4)) || !(offs = temps.take((size_t)tot * 4)))) return BMO_ERR_OOM;
    hipLaunchKernelGGL(hit_count_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)R->order.p, (const int32_t*)R->n_hitdet.p, (const int32_t*)R->n_nseg.p, n_nodes,
                       nd, nsub, cnt ? (int32_t*)cnt->p : nullptr, d_tail->shards);
    if (nd == 0) return BMO_OK;
    CUB_TRY(temps, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)cnt->p, (int32_t*)offs->p, (int)tot, stream));
    if ((rc = R->det_data.alloc((size_t)std::max<int64_t>(bound, 1) * 72)) || (rc = R->det_node.alloc((size_t)std::max<int64_t>(bound, 1) * 4))) return rc;
    hipLaunchKernelGGL(hit_gather_kernel, dim3(nb), dim3(256), 0, stream, (const int32_t*)R->order.p, (const int32_t*)R->n_hitdet.p, (const double*)R->n_hit.p,
                       n_nodes, nsub, (const int32_t*)offs->p, bound, (double*)R->det_data.p, (int32_t*)R->det_node.p, &d_tail->ctr.overflow, nd, d_tail->det_off);
    return BMO_OK;
}

// object kind recorded into every detector slot (bmo_trace_result::det_kind)
void note_detector_kinds(const bmo_scene* scene, bmo_trace_result* R) {
    R->det_kind.assign((size_t)R->n_detectors, -1);
    const bmo_object* obj = reinterpret_cast<const bmo_object*>(scene->blob.data() + scene->hdr.off_objects);
    for (int i = 0; i < scene->hdr.n_objects; ++i) {
        const int k = obj[i].kind, d = obj[i].detector;
        if ((k == BMO_OBJ_SPOTDETECTOR || k == BMO_OBJ_PSFDETECTOR || k == BMO_OBJ_PHOTODETECTOR) && d >= 0 && d < R->n_detectors)
            R->det_kind[(size_t)d] = (R->det_kind[(size_t)d] == -1 || R->det_kind[(size_t)d] == k) ? k : -2;  // -2: objects of two kinds
    }
}

OldSolution old_solution_of(const bmo_trace_result* prev) {
    OldSolution o{};
    o.nseg = (const int32_t*)prev->n_nseg.p;
    o.status = (const int32_t*)prev->n_status.p;
    o.first_child = (const int32_t*)prev->rt_first_child.p;
    o.rec_start = (const int32_t*)prev->rt_rec_start.p;
    o.rec_obj = (const int32_t*)prev->rt_rec_obj.p;
    o.aux = (const double*)prev->n_aux.p;
    o.rec_loc = (const int64_t*)prev->rt_rec_loc.p;
    o.chunks = (const OldChunk*)prev->rt_chunks.p;
    return o;
}

// The chunks of a launch over C.cur: the next launch's chunk first, then the in-place levels (the levels no wave reaches go back to the
// arena after the launch: marks[q] is the arena behind nxt and q levels).  Out of memory for a level lowers plan.n_fuse to what fits.
int alloc_launch_chunks(const KindInfo& K, ChunkArena& arena, bmo_trace_result* R, LaunchPlan& plan, bool has_split, LaunchChunks& C, ChunkArena::Mark* marks) {
    int rc;
    const int64_t m = C.cur.count;
    const bool sweep = plan.sweep_lanes > 0;
    if ((rc = arena.alloc((has_split ? 2 * m : m) + plan.inwave_cap + (plan.keep_kids ? m : 0), C.nxt))) return rc;
    C.wl = nullptr;
    if (arena.keep_log && plan.n_fuse > 1) {
        auto b = std::make_unique<DevBuf>();
        // one byte per wave of the GRID, not of the batch: the tail waves of the last workgroup (no record, j >= m) note their level too.
        // A sweep launch notes it per slot (a wave's slots are not consecutive there).
        if ((rc = b->alloc(sweep ? (size_t)m : (size_t)plan.n_blocks * (BMO_BLOCK / 64)))) return rc;
        C.wl = static_cast<uint8_t*>(b->p);
        R->wave_last.push_back(std::move(b));
    }
    marks[0] = arena.mark();
    for (int q = 0; q < (K.gauss ? plan.n_fuse : plan.n_fuse - 1); ++q) {
        if (!arena.keep_log && q > (K.gauss ? 1 : 0)) {
            // nobody reads the log: a lane's in-place record is dead once it has been read back, one chunk serves all levels (a beamlet's
            // step writes its next rays while the hits of the level it reads are still being filled in: two chunks, taken in turns)
            C.inner[q] = C.inner[K.gauss ? (q & 1) : 0];
            continue;
        }
        if ((rc = arena.alloc(m, C.inner[q]))) {
            if (rc != BMO_ERR_OOM || q == 0) return rc;
            plan.n_fuse = K.gauss ? q : q + 1;  // no room for this many in-place levels: fuse the ones that fit (the launch before fused fewer, too)
            break;
        }
        C.inner[q].count = m;  // same slot numbering as cur; records of beams that ended earlier are marked node = -1
        C.inner[q].wl = C.wl;
        C.inner[q].level = q + 1;
        C.inner[q].wl_shift = sweep ? 0 : plan.lane_shift;
        marks[q + 1] = arena.mark();
    }
    C.n_inner = K.gauss ? plan.n_fuse : plan.n_fuse - 1;
    return BMO_OK;
}

// wall-clock laps of a solve's phases on stderr (BMO_DEBUG)
struct PhaseClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!dbg_on()) return;
        const auto t = std::chrono::steady_clock::now();
        DBG("phase %-10s %.3f ms", what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};

// One turn of the step loop: plans the launch over C.cur, gives it its chunks, node slots and buffers, launches it and waits, then books
// what it made: the log's chunks (or their room back to the pool), C.cur = the next launch's records, R->n_nodes, R->n_steps.
int step_once(DevCtx& ctx, const KindInfo& K, bmo_scene* scene, const char* dblob, bmo_device_batch* batch, const bmo_trace_opts* opts, const SolveSwitches& sw,
              bmo_trace_result* R, bmo_trace_result* prev, const StepKernels& kern, ChunkArena& arena, NodeTable& nodes, const DevBuf& tbits, LaunchBufs& bufs,
              TailBlock* d_tail, LaunchChunks& C) {
    int rc;
    // bounces per launch: fewer launches and host round trips; holes instead of compaction inside a launch.  BMO_FUSE=1 (BMO_FUSE_GAUSS=1)
    // restores one launch per bounce level.
    // measured on C1-C5: 8 levels per launch beat 4 by 1-4 % at 10^6 beams and by 8-10 % below 10^5; with per-wave loops 16 beat 8 by
    // another 1-3 %, and 32 beat 16 by 1-2.5 % (config C2 reaches its splitter, level 17, in the first launch: 2 launches instead of 3).
    // The GaussianBeamlet kernels need one in-place chunk more than they fuse levels (step_kernel_gauss): one level fewer.
    const int fuse_max = std::max(1, std::min(K.gauss ? MAX_FUSE - 1 : MAX_FUSE, K.gauss ? sw.fuse_gauss : sw.fuse));
    const int steps = R->n_steps;  // launches so far = the number of this one
    const int64_t n_nodes = R->n_nodes;
    hipStream_t stream = ctx.stream;
    const Counters& h_ctr = *ctx.pinned;
    // a sweep (bmo_trace_sweep): R->n_configs configurations, R->d_root_cfg the configuration of every root; lanes find their slots through
    // the map built before the launch (StepParams::sweep)
    const bool has_split = scene->hdr.has_splitter != 0, sweep = R->n_configs > 0, keep_log = arena.keep_log;
    const int64_t m = C.cur.count;
    LaunchPlan plan = plan_launch(m, fuse_max, keep_log, arena.rec_bytes, has_split, kern.inw || K.gauss, R->n_configs);
    if (plan.sweep_lanes >= ((int64_t)1 << 31)) return fail(BMO_ERR_UNSUPPORTED, "sweep launch of more than 2^31 lanes: fewer roots per call");
    ChunkArena::Mark marks[MAX_FUSE];  // arena state behind nxt [0] and behind every in-place level [q + 1]
    if ((rc = alloc_launch_chunks(K, arena, R, plan, has_split, C, marks))) return rc;
    if (has_split && (rc = nodes.grow(n_nodes + 2 * m + 2 * plan.inwave_cap, stream))) return rc;
    if ((rc = bufs.fit(K, plan, m, arena.rec_bytes))) return rc;
    StepParams P;
    fill_step_params(P, K, scene, dblob, opts, C, plan, bufs, nodes.arrays(tbits), prev ? old_solution_of(prev) : OldSolution{}, &d_tail->ctr, d_tail->shards, steps, n_nodes);
    if (knobs().lpt && !sweep && steps == 0 && plan.lane_shift == 6 && plan.n_blocks >= 64 && (rc = tile_order_feedback(P, batch, prev, plan.n_blocks, stream))) return rc;
#if defined(BMO_DEV_TIMELINE)
    DevBuf tl_buf;
    if (sw.timeline && !sweep) {
        if ((rc = tl_buf.alloc((size_t)plan.n_waves * 16 + 64))) return rc;
        HIP_TRY(hipMemsetAsync(tl_buf.p, 0, tl_buf.bytes, stream));
        P.tl = (unsigned long long*)tl_buf.p;
    }
#endif
    DevBuf sw_map;  // (P.sweep shares its room with P.old: set for sweeps only)
    if (sweep) {
        if ((rc = build_sweep_lane_map(R, C.cur, plan.sweep_lanes, &d_tail->ctr, stream, sw_map))) return rc;
        P.sweep = SweepLanes{(const int32_t*)sw_map.p, (const int32_t*)R->d_root_cfg.p, scene->stride};
    }
    DBG("step %d launching m=%lld, %d records per wave", steps, (long long)m, 1 << plan.lane_shift);
    if ((rc = launch_step(ctx, kern, plan, P, steps, &d_tail->ctr, sw.wide_min_waves))) return rc;
#if defined(BMO_DEV_TIMELINE)
    if (P.tl && (rc = print_timeline(P.tl, (size_t)plan.n_waves, steps))) return rc;
#endif
    const unsigned long long produced = h_ctr.next_count[steps & 1];
    DBG("step %d done next=%llu nodes=%llu deepest in-place level %llu of %d", steps, produced, h_ctr.node_count, h_ctr.max_level[steps & 1], plan.n_fuse);
    R->n_steps = steps + 1;
    if (h_ctr.overflow) return fail(BMO_ERR_INTERNAL, "queue overflow (internal capacity bound violated)");
    if (h_ctr.sweep_mixed) return fail(BMO_ERR_INTERNAL, "sweep: a wave held records of more than one configuration (lane map violated)");
    if (keep_log) {
        const int used = (int)std::min<unsigned long long>(h_ctr.max_level[steps & 1], (unsigned long long)(plan.n_fuse - 1));  // in-place levels reached
        R->chunks.push_back(C.cur);
        for (int q = 0; q < used; ++q) R->chunks.push_back(C.inner[q]);
        // the levels behind them were never touched: their room goes back to the arena
        // (the GaussianBeamlet kernels' extra level is always given back; the launch has completed: nothing in flight touches these blocks)
        if (used < C.n_inner) arena.rewind(marks[used]);
    } else {  // the launch above has completed (counter read-back): its input and in-place levels are dead
        arena.drop(C.cur);
        if (K.gauss || plan.n_fuse > 1) arena.drop(C.inner[0]);
        if (K.gauss && plan.n_fuse > 1) arena.drop(C.inner[1]);
    }
    C.nxt.count = (int64_t)produced;  // (planes are strided by cap, so the chunk keeps its footprint)
    R->n_nodes = (int64_t)h_ctr.node_count;
    if (opts->max_beams > 0 && R->n_nodes > (int64_t)opts->max_beams)
        return fail(BMO_ERR_LIMIT, "beam tree exceeds bmo_trace_opts.max_beams (" + std::to_string(R->n_nodes) + " beams after " + std::to_string(R->n_steps) +
                                       " launches): a splitter facing a mirror?");
    C.cur = C.nxt;
    return BMO_OK;
}

// the step kernels' time of a solve, from the event pair around every launch
int sum_step_times(const DevCtx& ctx, int steps, bool gaps, double& kernel_ms) {
    kernel_ms = 0;
    for (int q = 0; q < steps; ++q) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ctx.step_ev[2 * q], ctx.step_ev[2 * q + 1]));
        kernel_ms += ms;
        DBG("step %d kernel %.3f ms", q, ms);
        if (q + 1 < steps && gaps) {  // diagnosis: device idle time between two step launches (host round trip)
            float gap = 0;
            (void)hipEventElapsedTime(&gap, ctx.step_ev[2 * q + 1], ctx.step_ev[2 * q + 2]);
            fprintf(stderr, "[bmo] step %d kernel %.3f ms, gap to the next launch %.3f ms\n", q, ms, gap);
        }
    }
    return BMO_OK;
}

// Everything behind the last launch: the canonical order, the segment count and the detector tables, all queued behind ONE
// synchronisation at the end.  The temporaries stay alive until then (`temps`: a block that went back to the pool could be handed to a
// view running on another stream); the tail block is read back last and unpacked into R.  Records ctx.ev[3] behind the queued work.
int finish_solve(DevCtx& ctx, bmo_trace_result* R, int nsub, int64_t n, int64_t n_nodes, const DevBuf& tbits, const SolveSwitches& sw, TailBlock* d_tail,
                 PhaseClock& clock) {
    int rc;
    hipStream_t stream = ctx.stream;
    Temps temps;
    const int nd = R->n_detectors;
    R->det_count.assign(nd, 0);
    R->det_offset.assign(nd, 0);
    if ((rc = order_nodes(R, n, n_nodes, ctx.pinned->max_depth, tbits, sw.force_sort_order, sw.force_deep_order, stream, temps))) return rc;
    clock.lap("order");
    // segments = sum of the beams' segment counts (chunk counts include the holes of fused levels)
    if (n_nodes > 0 && (rc = count_and_gather_hits(R, nsub, n, n_nodes, d_tail, stream, temps))) return rc;
    TailBlock& h_tail = *ctx.tail_back;
    HIP_TRY(hipMemcpyAsync(&h_tail, d_tail, tail_bytes(nd), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(ctx.ev[3], stream));
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());
    clock.lap("hits");
    if (h_tail.ctr.overflow) return fail(BMO_ERR_INTERNAL, "hit table overflow (internal capacity bound violated)");
    unsigned long long tot = 0, seg = 0;
    for (int q = 0; q < 64; ++q) tot += h_tail.shards[(size_t)q * 16], seg += h_tail.shards[(size_t)q * 16 + 1];
    R->calls = tot;
    R->n_records = (int64_t)seg;
    for (int d = 0; d < nd && n_nodes > 0; ++d) {
        R->det_offset[d] = h_tail.det_off[d];
        R->det_count[d] = h_tail.det_off[d + 1] - h_tail.det_off[d];
    }
    return BMO_OK;
}

int run_trace(const KindInfo& K, bmo_scene* scene, bmo_device_batch* batch, const bmo_trace_opts* opts, bmo_trace_result* R, bmo_trace_result* prev) {
    const int device = batch->device;
    if (prev) {
        if (prev->device != device) return fail(BMO_ERR_INVALID, "retrace: the previous solution lives on another device");
        if (prev->kind != K.kind || prev->n_roots != batch->n)
            return fail(BMO_ERR_INVALID, "retrace: batch does not match the previous solution (root count / beam kind)");
    }
    HIP_TRY(hipSetDevice(device));
    const SolveSwitches sw = read_switches().solve;  // (read at the start of every solve: the tests switch these between solves)
    int rc = BMO_OK;
    const char* dblob = scene->device_blob(device, rc);
    if (rc) return rc;
    const int64_t n = batch->n;
    const bool has_split = scene->hdr.has_splitter != 0;
    R->device = device;
    R->kind = K.kind;
    R->n_roots = n;
    R->n_detectors = scene->hdr.n_detectors;
    note_detector_kinds(scene, R);
    R->nd = K.nd;
    R->abi_planes = K.abi_planes;

    PhaseClock clock;
    DevCtx* ctxp = nullptr;
    if ((rc = device_ctx(device, ctxp))) return rc;
    DevCtx& ctx = *ctxp;
    std::lock_guard<std::mutex> one_trace_per_device(ctx.busy);
    hipStream_t stream = ctx.stream;
    HIP_TRY(hipEventRecord(ctx.ev[2], stream));
    // Every exit path — the error returns too — waits for what has been queued BEFORE the temporaries of this function go back to the
    // shared pools: a kernel or copy still in flight must not write into a block another host thread has been handed.
    // While `hold` lives, blocks released on this thread are parked in it; its destructor (it is declared before every temporary, so it
    // runs after theirs) synchronises the stream and only then hands them to the pools.  The phases called below inherit that: their
    // temporaries are released on this thread while `hold` is alive.
    PoolHold hold(stream);

    // node arrays: roots + room for children (grown on demand)
    // Children need node slots, and every launch must have room for two per record it traces (any record may split).  One splitter per
    // ray (3 n beams) then asks for 7 n slots before the launch that follows the split; growing the tables there costs a device copy of
    // every node array (0.3 ms of a 6 ms solve of config C2), so moderate batches get that room up front.  Larger ones grow on demand.
    NodeTable nodes{R, K.nsub, prev != nullptr};
    if ((rc = nodes.alloc(has_split ? (n <= ((int64_t)1 << 22) ? 7 * n + 64 : 3 * n + 64) : n))) return rc;
    DevBuf tbits_buf;  // NodeArrays::tbits (allocated below when the scene has a splitter)

    const bool keep_log = opts->record_segments != 0;
    R->has_log = keep_log;
    const size_t rec_bytes = (size_t)K.nd * 8 + (size_t)NI * 4;
    ChunkArena arena{R->arena, (size_t)K.nd * 8, rec_bytes, std::max<size_t>((size_t)n * rec_bytes * 6, (size_t)1 << 20), keep_log};

    if (R->n_detectors > MAX_DETECTORS) return fail(BMO_ERR_UNSUPPORTED, "more than 1023 detectors");
    // counters, call-counter shards, segment count and detector offsets: one block, set by one copy (the image is zero but for the node count)
    DevBuf tail_buf;
    if ((rc = tail_buf.alloc(sizeof(TailBlock)))) return rc;
    TailBlock* const d_tail = static_cast<TailBlock*>(tail_buf.p);
    *ctx.pinned = Counters{{0, 0}, (unsigned long long)n, 0, 0, {0, 0}};  // pinned: the per-step read-back does not go through a staging copy
    ctx.tail_img->ctr.node_count = (unsigned long long)n;
    HIP_TRY(hipMemcpyAsync(d_tail, ctx.tail_img, tail_bytes(R->n_detectors), hipMemcpyHostToDevice, stream));

    LaunchChunks C;
    if ((rc = arena.alloc(n, C.cur))) return rc;
    C.cur.count = n;
    if (prev && (rc = build_retrace_tables(prev, stream))) return rc;  // (step_once hands them to the kernels: old_solution_of)
    if (has_split && n > 0 && (rc = tbits_buf.alloc((size_t)n * 8))) return rc;
    if (n > 0) {
        // a retrace re-walks the stored first ray whatever r_max says (System.jl:197); root j re-walks old node j
        hipLaunchKernelGGL(K.init_roots, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)batch->planes.p,
                           (const double*)(batch->perm.p ? batch->binned.p : batch->planes.p), (const int32_t*)batch->li.p, (const int32_t*)batch->perm.p, n, C.cur,
                           nodes.arrays(tbits_buf), prev ? 0x7fffffff : opts->r_max, (int32_t)batch->n_planes);
        if (prev) hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (int32_t*)R->n_old.p, n);
    }
    clock.lap("setup");
    DBG("roots initialised n=%lld blob=%u", (long long)n, (uint32_t)scene->blob.size());
    if (dbg_on()) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipGetLastError());
        DBG("init kernel done");
    }
    StepKernels kern;
    const int ext = scene->hdr.has_bvh() ? 3 : (scene->hdr.has_asphere ? 2 : (scene->hdr.has_meniscus ? 1 : 0));
    if ((rc = K.select(ext, prev != nullptr, R->n_configs > 0, kern))) return rc;

    R->n_nodes = n;
    R->n_steps = 0;
    LaunchBufs bufs;
    while (C.cur.count > 0)
        if ((rc = step_once(ctx, K, scene, dblob, batch, opts, sw, R, prev, kern, arena, nodes, tbits_buf, bufs, d_tail, C))) return rc;
    if ((rc = sum_step_times(ctx, R->n_steps, sw.gaps, R->kernel_ms))) return rc;
    clock.lap("steps");
    if (batch->cost_valid && batch->tile_n > 0 && batch->tile_cost.p && !R->tile_cost.alloc((size_t)batch->tile_n * 4)) {  // (best effort)
        if (hipMemcpyAsync(R->tile_cost.p, batch->tile_cost.p, (size_t)batch->tile_n * 4, hipMemcpyDeviceToDevice, stream) == hipSuccess) R->tile_n = batch->tile_n;
    }
    if ((rc = finish_solve(ctx, R, K.nsub, n, R->n_nodes, tbits_buf, sw, d_tail, clock))) return rc;
    float tms = 0;
    HIP_TRY(hipEventElapsedTime(&tms, ctx.ev[2], ctx.ev[3]));
    R->total_ms = tms;
    return BMO_OK;
}

// the beam-kind dispatch, in one place
int trace_by_kind(bmo_scene* scene, bmo_device_batch* batch, const bmo_trace_opts* opts, bmo_trace_result* R, bmo_trace_result* prev) {
    if (batch->kind == BMO_BEAM_RAY) return run_trace(kind_info<BMO_BEAM_RAY>(), scene, batch, opts, R, prev);
    if (batch->kind == BMO_BEAM_POLARIZED) return run_trace(kind_info<BMO_BEAM_POLARIZED>(), scene, batch, opts, R, prev);
    if (batch->kind == BMO_BEAM_GAUSSIAN) return run_trace(kind_info<BMO_BEAM_GAUSSIAN>(), scene, batch, opts, R, prev);
    return fail(BMO_ERR_UNSUPPORTED, "beam kind not built yet");
}
