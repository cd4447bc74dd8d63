// bmo_result_view.inc.hpp — a finished solution on its way to the host (included by bmo_engine.hip at file scope, behind the handle structs
// and bmo_trace_host.inc.hpp, whose iota_kernel it shares).  The kernels only these entry points launch come first, then the phases of
// bmo_result_view_select, then the entry points:
//   rank_kernel, canon_nodes_kernel, dst_base_kernel, last_records_kernel, hit_columns_kernel, order_records_kernel
//   view_node_tables, view_hit_tables, view_records, fill_view     the four phases of a view
//   bmo_result_device_hits, bmo_result_copy_hits, bmo_result_timing, bmo_result_counts, bmo_result_view_select, bmo_result_view,
//   bmo_result_copy_hit_columns
namespace {

// Node tables in the ABI's canonical order, built on the device (the host used to loop over 3 M nodes per C2 solve):
//   rank[order[i]] = i, then for canonical node i (id nd = order[i]): root, parent's rank, nseg, status, aux; the transmitted child
//   (path bit 0) writes itself as first_child of its parent — siblings are adjacent in BFS order, no atomics.
__global__ void rank_kernel(const int32_t* __restrict__ order, int64_t n, int32_t* __restrict__ rank) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rank[order[i]] = (int32_t)i;
}
__global__ void canon_nodes_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ rank, int64_t n, int gaussian, const int32_t* __restrict__ root,
                                   const int32_t* __restrict__ parent, const int32_t* __restrict__ nseg, const int32_t* __restrict__ status,
                                   const unsigned long long* __restrict__ key, const double* __restrict__ lambda, const double* __restrict__ aux,
                                   int32_t* __restrict__ o_root, int32_t* __restrict__ o_parent, int32_t* __restrict__ o_first_child, int32_t* __restrict__ o_nseg,
                                   int32_t* __restrict__ o_status, double* __restrict__ o_aux) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t nd = order[i];
    const int32_t p = parent[nd];
    o_root[i] = root[nd];
    o_parent[i] = p < 0 ? -1 : rank[p];
    o_nseg[i] = nseg[nd];
    o_status[i] = status[nd];
    if (gaussian) {
        o_aux[4 * i + 0] = aux[4 * (int64_t)nd + 1];
        o_aux[4 * i + 1] = aux[4 * (int64_t)nd + 2];
        o_aux[4 * i + 2] = aux[4 * (int64_t)nd + 3];
        o_aux[4 * i + 3] = lambda[nd];
    } else {
        o_aux[4 * i + 0] = lambda[nd];
        o_aux[4 * i + 1] = o_aux[4 * i + 2] = o_aux[4 * i + 3] = 0.0;
    }
    if (p >= 0 && !(key[nd] & 1ull)) o_first_child[rank[p]] = (int32_t)i;
}
// dst_base[nd] = first record of node id nd in the node-major record order
__global__ void dst_base_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ first_rec, int64_t n, int32_t* __restrict__ dst_base) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst_base[order[i]] = first_rec[i];
}
// Last segment of every beam (last(rays(beam)), Beam.jl:79): record (node, k = nseg - 1) goes to column rank[node].
__global__ void last_records_kernel(Chunk c, int planes, const int32_t* __restrict__ rank, const int32_t* __restrict__ nseg, int64_t nn, double* __restrict__ rec,
                                    int32_t* __restrict__ obj, int32_t* __restrict__ shape) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.count) return;
    const int32_t nd = chunk_node(c, j);
    if (nd < 0) return;  // hole of a fused level
    if (c.i[I_K * c.cap + j] != nseg[nd] - 1) return;
    const int64_t dst = rank[nd];
    for (int p = 0; p < planes; ++p) rec[(int64_t)p * nn + dst] = c.d[(int64_t)p * c.cap + j];
    obj[dst] = c.i[I_OBJ * c.cap + j];
    shape[dst] = c.i[I_SHAPE * c.cap + j];
}
// the leading n_cols columns of a [n][9] hit table, packed (a Spotdetector keeps x, y only: 16 of the 72 bytes)
__global__ void hit_columns_kernel(const double* __restrict__ src, int64_t n, int n_cols, double* __restrict__ dst) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_cols) return;
    const int64_t i = t / n_cols;
    dst[t] = src[i * 9 + (t - i * n_cols)];
}

// Segment log -> the ABI's node-major order (bmo_trace_result_view.rec): record j of a step chunk goes to first_rec(node) + k.
// Done in HBM so that the host receives ONE contiguous copy per table instead of re-ordering 10^7 records itself.
__global__ void order_records_kernel(Chunk c, int planes, const int32_t* __restrict__ dst_base, int64_t nr, double* __restrict__ rec,
                                     int32_t* __restrict__ obj, int32_t* __restrict__ shape) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.count) return;
    const int32_t nd = chunk_node(c, j);
    if (nd < 0) return;  // hole of a fused level
    const int64_t dst = (int64_t)dst_base[nd] + c.i[I_K * c.cap + j];
    for (int p = 0; p < planes; ++p) rec[(int64_t)p * nr + dst] = c.d[(int64_t)p * c.cap + j];
    obj[dst] = c.i[I_OBJ * c.cap + j];
    shape[dst] = c.i[I_SHAPE * c.cap + j];
}

// ---- the canonical node tables: built on the device, one pinned copy each; made by the first view of a result
int view_node_tables(bmo_trace_result* r) {
    if (r->nodes_viewed) return BMO_OK;
    const int64_t nn = r->n_nodes;
    const unsigned nb = (unsigned)((nn + 255) / 256);
    const size_t n1 = (size_t)std::max<int64_t>(nn, 1);
    DevBuf d_root, d_parent, d_fc, d_nseg, d_status, d_aux;
    Temps tmp;
    int rc;
    if ((rc = r->c_rank.alloc(n1 * 4)) || (rc = r->c_first_rec.alloc(n1 * 4)) || (rc = d_root.alloc(n1 * 4)) || (rc = d_parent.alloc(n1 * 4)) ||
        (rc = d_fc.alloc(n1 * 4)) || (rc = d_nseg.alloc(n1 * 4)) || (rc = d_status.alloc(n1 * 4)) || (rc = d_aux.alloc(n1 * 32)) ||
        (rc = r->h_root.alloc(n1 * 4)) || (rc = r->h_parent.alloc(n1 * 4)) || (rc = r->h_first_child.alloc(n1 * 4)) || (rc = r->h_first_rec.alloc(n1 * 4)) ||
        (rc = r->h_last_rec.alloc(n1 * 4)) || (rc = r->h_nseg.alloc(n1 * 4)) || (rc = r->h_status.alloc(n1 * 4)) || (rc = r->h_aux.alloc(n1 * 32)))
        return rc;
    if (nn > 0) {
        hipLaunchKernelGGL(rank_kernel, dim3(nb), dim3(256), 0, 0, (const int32_t*)r->order.p, nn, (int32_t*)r->c_rank.p);
        HIP_TRY(hipMemsetAsync(d_fc.p, 0xFF, (size_t)nn * 4, 0));
        hipLaunchKernelGGL(canon_nodes_kernel, dim3(nb), dim3(256), 0, 0, (const int32_t*)r->order.p, (const int32_t*)r->c_rank.p, nn,
                           r->kind == BMO_BEAM_GAUSSIAN ? 1 : 0, (const int32_t*)r->n_root.p, (const int32_t*)r->n_parent.p, (const int32_t*)r->n_nseg.p,
                           (const int32_t*)r->n_status.p, (const unsigned long long*)r->n_key.p, (const double*)r->n_lambda.p, (const double*)r->n_aux.p,
                           (int32_t*)d_root.p, (int32_t*)d_parent.p, (int32_t*)d_fc.p, (int32_t*)d_nseg.p, (int32_t*)d_status.p, (double*)d_aux.p);
        CUB_TRY(tmp, hipcub::DeviceScan::ExclusiveSum(cub_tmp, cub_bytes, (const int32_t*)d_nseg.p, (int32_t*)r->c_first_rec.p, (int)nn, (hipStream_t)0));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(r->h_root.p, d_root.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_parent.p, d_parent.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_first_child.p, d_fc.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_first_rec.p, r->c_first_rec.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_nseg.p, d_nseg.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_status.p, d_status.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_aux.p, d_aux.p, (size_t)nn * 32, hipMemcpyDeviceToHost, 0));
        // LAST view: record i belongs to node i (d_root is free again once its copy is queued: the stream keeps the order)
        hipLaunchKernelGGL(iota_kernel, dim3(nb), dim3(256), 0, 0, (int32_t*)d_root.p, nn);
        HIP_TRY(hipMemcpyAsync(r->h_last_rec.p, d_root.p, (size_t)nn * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipStreamSynchronize(0));  // the staging buffers go back to the pool when this scope ends
    }
    r->nodes_viewed = true;
    return BMO_OK;
}

// ---- the hit tables: queued behind the node tables, completed by the synchronisation at the end of bmo_result_view_select
int view_hit_tables(bmo_trace_result* r) {
    if (r->hits_viewed) return BMO_OK;
    int64_t tot = 0;
    for (int d = 0; d < r->n_detectors; ++d) tot += r->det_count[d];
    int rc;
    if ((rc = r->h_det.alloc((size_t)tot * 72)) || (rc = r->h_det_node.alloc((size_t)tot * 4))) return rc;
    if (tot > 0) {
        HIP_TRY(hipMemcpyAsync(r->h_det.p, r->det_data.p, (size_t)tot * 72, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_det_node.p, r->det_node.p, (size_t)tot * 4, hipMemcpyDeviceToHost, 0));
    }
    r->hits_viewed = true;
    return BMO_OK;
}

// ---- the records in mode 1 (the last segment of every beam) or 2 (the whole log): re-ordered on the device, then one copy per table
int view_records(bmo_trace_result* r, int mode) {
    const int64_t nn = r->n_nodes, nr = r->n_records;
    const int P = r->abi_planes;
    const unsigned nb = (unsigned)((nn + 255) / 256);
    const int64_t cols = mode == 2 ? nr : nn;  // records on the host
    int rc;
    if ((rc = r->h_rec.alloc((size_t)P * cols * 8)) || (rc = r->h_rec_obj.alloc((size_t)cols * 4)) || (rc = r->h_rec_shape.alloc((size_t)cols * 4))) return rc;
    if (cols > 0) {
        DevBuf d_base, d_rec, d_obj, d_shape;
        if ((rc = d_rec.alloc((size_t)P * cols * 8)) || (rc = d_obj.alloc((size_t)cols * 4)) || (rc = d_shape.alloc((size_t)cols * 4))) return rc;
        // every beam has a last record and every (node, k) of the log exactly one record: both forms write every column
        // (a hole in the tables would be a bug of the log, which test_selective_views / compare() would show as garbage)
        if (mode == 2) {
            if ((rc = d_base.alloc((size_t)nn * 4))) return rc;
            hipLaunchKernelGGL(dst_base_kernel, dim3(nb), dim3(256), 0, 0, (const int32_t*)r->order.p, (const int32_t*)r->c_first_rec.p, nn, (int32_t*)d_base.p);
        }
        for (const Chunk& c : r->chunks) {
            if (c.count <= 0) continue;
            if (mode == 2)
                hipLaunchKernelGGL(order_records_kernel, dim3((unsigned)((c.count + 255) / 256)), dim3(256), 0, 0, c, P, (const int32_t*)d_base.p, nr,
                                   (double*)d_rec.p, (int32_t*)d_obj.p, (int32_t*)d_shape.p);
            else
                hipLaunchKernelGGL(last_records_kernel, dim3((unsigned)((c.count + 255) / 256)), dim3(256), 0, 0, c, P, (const int32_t*)r->c_rank.p,
                                   (const int32_t*)r->n_nseg.p, nn, (double*)d_rec.p, (int32_t*)d_obj.p, (int32_t*)d_shape.p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(r->h_rec.p, d_rec.p, (size_t)P * cols * 8, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_rec_obj.p, d_obj.p, (size_t)cols * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipMemcpyAsync(r->h_rec_shape.p, d_shape.p, (size_t)cols * 4, hipMemcpyDeviceToHost, 0));
        HIP_TRY(hipStreamSynchronize(0));  // the staging buffers go back to the pool when this scope ends
    }
    r->rec_mode = mode;
    return BMO_OK;
}

// ---- the view struct: the tables of mode `show` (0: no records), the hit tables when `what` asks for them
void fill_view(bmo_trace_result* r, uint32_t what, int show, bmo_trace_result_view* v) {
    std::memset(v, 0, sizeof *v);
    v->n_roots = r->n_roots;
    v->n_nodes = r->n_nodes;
    v->n_records = show == 2 ? r->n_records : (show == 1 ? r->n_nodes : 0);  // 0 when the log was not kept (record_segments = 0) or not asked for
    v->n_intersect_calls = (int64_t)r->calls;
    v->n_steps = r->n_steps;
    v->beam_kind = r->kind;
    v->rec_planes = r->abi_planes;
    v->n_detectors = r->n_detectors;
    v->node_root = r->h_root.as<int32_t>();
    v->node_parent = r->h_parent.as<int32_t>();
    v->node_first_child = r->h_first_child.as<int32_t>();
    v->node_first_rec = show == 1 ? r->h_last_rec.as<int32_t>() : r->h_first_rec.as<int32_t>();
    v->node_nseg = r->h_nseg.as<int32_t>();
    v->node_status = r->h_status.as<int32_t>();
    v->node_aux = r->h_aux.as<double>();
    if (show) {
        v->rec_obj = r->h_rec_obj.as<int32_t>();
        v->rec_shape = r->h_rec_shape.as<int32_t>();
        v->rec = r->h_rec.as<double>();
    }
    v->det_count = r->det_count.data();
    v->det_offset = r->det_offset.data();
    if (what & BMO_VIEW_HITS) {
        v->det_node = r->h_det_node.as<int32_t>();
        v->det_data = r->h_det.as<double>();
    }
}

}  // namespace

extern "C" {

int bmo_result_device_hits(bmo_trace_result* r, int32_t det, const double** data, int64_t* count) {
    if (!r || det < 0 || det >= r->n_detectors) return fail(BMO_ERR_INVALID, "bad detector");
    *count = r->det_count[det];
    *data = r->det_data.p ? static_cast<const double*>(r->det_data.p) + 9 * r->det_offset[det] : nullptr;
    return BMO_OK;
}

int bmo_result_copy_hits(bmo_trace_result* r, int32_t det, double* dst, int64_t max_hits) {
    if (!r || det < 0 || det >= r->n_detectors) return fail(BMO_ERR_INVALID, "bad argument");
    const int64_t n = std::min<int64_t>(max_hits, r->det_count[det]);
    if (n <= 0) return BMO_OK;  // nothing to copy: an empty destination (NULL data pointer of a 0-row tensor) is fine
    if (!dst) return fail(BMO_ERR_INVALID, "null destination");
    HIP_TRY(hipSetDevice(r->device));
    HIP_TRY(hipMemcpy(dst, static_cast<const double*>(r->det_data.p) + 9 * r->det_offset[det], (size_t)n * 72, hipMemcpyDefault));
    return BMO_OK;
}

int bmo_result_timing(bmo_trace_result* r, double* k, double* t, int32_t* n) {
    if (!r) return fail(BMO_ERR_INVALID, "null result");
    if (k) *k = r->kernel_ms;
    if (t) *t = r->total_ms;
    if (n) *n = r->n_steps;
    return BMO_OK;
}

int bmo_result_counts(bmo_trace_result* r, int64_t* calls, int64_t* records, int64_t* nodes, int64_t* hits) {
    if (!r) return fail(BMO_ERR_INVALID, "null result");
    if (calls) *calls = (int64_t)r->calls;
    if (records) *records = r->n_records;
    if (nodes) *nodes = r->n_nodes;
    if (hits) {
        *hits = 0;
        for (int d = 0; d < r->n_detectors; ++d) *hits += r->det_count[d];
    }
    return BMO_OK;
}

int bmo_result_view_select(bmo_trace_result* r, uint32_t what, bmo_trace_result_view* v) {
    if (!r || !v) return fail(BMO_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->device));
    if (r->n_records >= ((int64_t)1 << 31)) return fail(BMO_ERR_UNSUPPORTED, "result view: more than 2^31 segments (node_first_rec is 32-bit)");
    int rc;
    if ((rc = view_node_tables(r))) return rc;
    if ((what & BMO_VIEW_HITS) && (rc = view_hit_tables(r))) return rc;
    // Which records come to the host: the whole log when asked for, else the last segments when asked for; a result keeps one of the two
    // (the whole log already there serves no LAST view: its node_first_rec differs).
    const int want_mode = !r->has_log ? 0 : ((what & BMO_VIEW_SEGMENTS) ? 2 : ((what & BMO_VIEW_LAST_SEGMENT) ? 1 : 0));
    if (want_mode != 0 && want_mode != r->rec_mode && !(want_mode == 1 && r->rec_mode == 2) && (rc = view_records(r, want_mode))) return rc;
    HIP_TRY(hipStreamSynchronize(0));
    // what this view shows: the whole log only when asked for it (or when nothing narrower was asked and it is there)
    const int show = (what & BMO_VIEW_SEGMENTS) ? (r->rec_mode == 2 ? 2 : 0) : ((what & BMO_VIEW_LAST_SEGMENT) ? (r->rec_mode == 1 ? 1 : 0) : 0);
    if ((what & BMO_VIEW_LAST_SEGMENT) && !(what & BMO_VIEW_SEGMENTS) && r->rec_mode == 2)
        return fail(BMO_ERR_INVALID, "result view: the whole log of this result is already on the host; ask for BMO_VIEW_SEGMENTS");
    fill_view(r, what, show, v);
    return BMO_OK;
}

int bmo_result_view(bmo_trace_result* r, bmo_trace_result_view* v) { return bmo_result_view_select(r, BMO_VIEW_HITS | BMO_VIEW_SEGMENTS, v); }

int bmo_result_copy_hit_columns(bmo_trace_result* r, int32_t det, int32_t n_cols, double* dst, int64_t max_hits) {
    if (!r || det < 0 || det >= r->n_detectors || n_cols < 1 || n_cols > 9) return fail(BMO_ERR_INVALID, "bad argument");
    const int64_t n = std::min<int64_t>(max_hits, r->det_count[det]);
    if (n <= 0) return BMO_OK;
    if (!dst) return fail(BMO_ERR_INVALID, "null destination");
    HIP_TRY(hipSetDevice(r->device));
    const double* src = static_cast<const double*>(r->det_data.p) + 9 * r->det_offset[det];
    hipPointerAttribute_t at{};
    const bool on_device = hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();  // a pageable host pointer makes the query fail: not an error here
    const unsigned grid = (unsigned)((n * n_cols + 255) / 256);
    if (on_device) {
        hipLaunchKernelGGL(hit_columns_kernel, dim3(grid), dim3(256), 0, 0, src, n, (int)n_cols, dst);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(0));
        return BMO_OK;
    }
    DevBuf packed;
    int rc = packed.alloc((size_t)n * n_cols * 8);
    if (rc) return rc;
    hipLaunchKernelGGL(hit_columns_kernel, dim3(grid), dim3(256), 0, 0, src, n, (int)n_cols, (double*)packed.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(dst, packed.p, (size_t)n * n_cols * 8, hipMemcpyDeviceToHost));
    return BMO_OK;
}

}  // extern "C"
