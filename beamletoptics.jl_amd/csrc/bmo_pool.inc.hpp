// bmo_pool.inc.hpp — memory of the host side (included by bmo_engine.hip inside its anonymous namespace, behind the step kernels; uses
// its fail()).  Nothing here launches a kernel.
//   PoolBlock, take_best_fit   a kept block; the ONE search both pools reuse blocks by
//   pool_take / pool_give / pool_release_all   the device pool
//   PoolHold                   releases deferred until a stream has been synchronised
//   DevBuf, HostBuf            a device block / a page-locked host block, back to its pool when it dies
//   cub_run, CUB_TRY           hipcub's two-call protocol
//   Temps, scratch_in          the temporaries of a stretch of queued work

// Device memory pool: hipMalloc/hipFree of the multi-GB segment log cost more than the trace itself, so
// freed blocks are kept per device and reused by the next trace (same sizes every call for a fixed batch).
struct PoolBlock {
    void* p;
    size_t bytes;
    int device;
};
// Takes the smallest block of `device` that holds `bytes` and is not much larger (a quarter + 4 KiB) out of `pool`, whose lock the caller
// holds; nullptr: none.  `got`: the block's size.
void* take_best_fit(std::vector<PoolBlock>& pool, size_t& pool_bytes, size_t bytes, int device, size_t& got) {
    int best = -1;
    for (int i = 0; i < (int)pool.size(); ++i) {
        const PoolBlock& b = pool[i];
        if (b.device != device || b.bytes < bytes || b.bytes > bytes + bytes / 4 + 4096) continue;
        if (best < 0 || b.bytes < pool[best].bytes) best = i;
    }
    if (best < 0) return nullptr;
    void* p = pool[best].p;
    got = pool[best].bytes;
    pool_bytes -= got;
    pool.erase(pool.begin() + best);
    return p;
}
std::mutex g_pool_mu;
std::vector<PoolBlock> g_pool;
size_t g_pool_bytes = 0;

void* pool_take(size_t bytes, int device, size_t& got) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    return take_best_fit(g_pool, g_pool_bytes, bytes, device, got);
}
void pool_give(void* p, size_t bytes, int device) {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    g_pool.push_back({p, bytes, device});
    g_pool_bytes += bytes;
}
void pool_release_all() {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto& b : g_pool) {
        (void)hipSetDevice(b.device);
        (void)hipFree(b.p);
    }
    (void)hipSetDevice(cur);
    g_pool.clear();
    g_pool_bytes = 0;
}

// Deferred release (run_trace): device and pinned blocks released on this thread while a PoolHold lives are parked in it and go
// back to the pools when it dies, after the stream has been synchronised.  PoolHold::Now lifts the deferral inside a scope whose
// releases are known to be safe at once (a chunk whose launch has completed, record_segments = 0).
struct PoolHold;
thread_local PoolHold* g_hold = nullptr;
void host_pool_give(void* p, size_t bytes);
struct PoolHold {
    hipStream_t stream;
    std::vector<PoolBlock> dev;
    std::vector<std::pair<void*, size_t>> host;
    PoolHold* prev;
    explicit PoolHold(hipStream_t s) : stream(s), prev(g_hold) { g_hold = this; }
    ~PoolHold() {
        g_hold = prev;
        (void)hipStreamSynchronize(stream);
        for (auto& b : dev) pool_give(b.p, b.bytes, b.device);
        for (auto& h : host) host_pool_give(h.first, h.second);
    }
    PoolHold(const PoolHold&) = delete;
    PoolHold& operator=(const PoolHold&) = delete;
    struct Now {
        PoolHold* saved;
        Now() : saved(g_hold) { g_hold = nullptr; }
        ~Now() { g_hold = saved; }
    };
};

// BMO_POOL_POISON (a test hook, DESIGN.md §2 "State independence"): every block handed out, recycled or fresh, is filled over its whole
// `bytes` with a word that cannot pass for data: a NaN as FP64 and as FP32, 2 147 016 365 as int32, and neither 0 nor -1 in any width,
// the two markers the engine sets itself with hipMemsetAsync.  The device is synchronised before and after the fill: the mode is
// deterministic and orders nothing that was not ordered already.
constexpr uint32_t POOL_POISON_WORD = 0x7FF8DEADu;
int poison_device_block(void* p, size_t bytes) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)p, (int)POOL_POISON_WORD, bytes / 4));
    for (size_t i = bytes & ~(size_t)3; i < bytes; ++i)  // the tail's bytes continue the word (little endian)
        HIP_TRY(hipMemsetD8((hipDeviceptr_t)((char*)p + i), (unsigned char)(POOL_POISON_WORD >> (8 * (i & 3))), 1));
    HIP_TRY(hipDeviceSynchronize());
    return BMO_OK;
}
void poison_host_block(void* p, size_t bytes) {
    for (size_t i = 0; i < bytes / 4; ++i) static_cast<uint32_t*>(p)[i] = POOL_POISON_WORD;
    for (size_t i = bytes & ~(size_t)3; i < bytes; ++i) static_cast<unsigned char*>(p)[i] = (unsigned char)(POOL_POISON_WORD >> (8 * (i & 3)));
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int device = 0;
    int alloc(size_t b) {
        release();
        if (b == 0) b = 16;
        (void)hipGetDevice(&device);
        size_t got = 0;
        if (void* q = pool_take(b, device, got)) {
            p = q;
            bytes = got;
            return knobs().pool_poison ? poison_device_block(p, bytes) : BMO_OK;
        }
        hipError_t e = hipMalloc(&p, b);
        if (e != hipSuccess) {
            pool_release_all();  // give cached blocks back and retry once
            e = hipMalloc(&p, b);
        }
        if (e != hipSuccess) {
            p = nullptr;
            return fail(BMO_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        bytes = b;
        return knobs().pool_poison ? poison_device_block(p, bytes) : BMO_OK;
    }
    void release() {
        if (p) {
            if (g_hold) g_hold->dev.push_back({p, bytes, device});
            else pool_give(p, bytes, device);
        }
        p = nullptr;
        bytes = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// Page-locked host memory for the tables bmo_result_view hands out: a D2H copy into pinned memory runs at PCIe speed, into
// pageable memory at a fraction of it.  Pinning costs more than the copy, so freed blocks are kept (up to a cap) and reused
// by the next view of a similar size.
constexpr size_t HOST_POOL_CAP = (size_t)16 << 30;
std::mutex g_hpool_mu;
std::vector<PoolBlock> g_hpool;
size_t g_hpool_bytes = 0;

void host_pool_give(void* p, size_t bytes) {
    std::unique_lock<std::mutex> lk(g_hpool_mu);
    if (g_hpool_bytes + bytes <= HOST_POOL_CAP) {
        g_hpool.push_back({p, bytes, 0});
        g_hpool_bytes += bytes;
    } else {
        lk.unlock();
        (void)hipHostFree(p);
    }
}

struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int alloc(size_t b) {
        release();
        if (b == 0) b = 16;
        {
            std::lock_guard<std::mutex> lk(g_hpool_mu);
            p = take_best_fit(g_hpool, g_hpool_bytes, b, 0, bytes);  // (host blocks are kept as device 0)
        }
        if (!p) {
            if (hipHostMalloc(&p, b, hipHostMallocDefault) != hipSuccess) {
                p = nullptr;
                return fail(BMO_ERR_OOM, "hipHostMalloc failed");
            }
            bytes = b;
        }
        if (knobs().pool_poison) poison_host_block(p, bytes);
        return BMO_OK;
    }
    void release() {
        if (!p) return;
        if (g_hold) g_hold->host.emplace_back(p, bytes);
        else host_pool_give(p, bytes);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    ~HostBuf() { release(); }
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
};

// hipcub's two-call protocol, written once: f(nullptr, bytes) asks for the size of the temporary storage, scratch(bytes) provides it
// (nullptr: out of memory, the error text is set), f(tmp, bytes) runs.  Errors map as in HIP_TRY; `what` names the call.
// The scratch decides how long the block lives: it must not go back to the pool while work queued on it may still run.
template <class Scratch, class F>
int cub_run(Scratch&& scratch, const char* what, F&& f) {
    size_t bytes = 0;
    hipError_t e = f(nullptr, bytes);
    if (e == hipSuccess) {
        void* tmp = scratch(bytes);
        if (!tmp) return BMO_ERR_OOM;
        e = f(tmp, bytes);
    }
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? BMO_ERR_OOM : BMO_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return BMO_OK;
}
// CUB_TRY(scratch, hipcub::Algorithm(cub_tmp, cub_bytes, ...)): the call is written once, with these two names for its first two arguments
#define CUB_TRY(scratch, call)                                                                                      \
    do {                                                                                                            \
        if (int rc_ = cub_run(scratch, #call, [&](void* cub_tmp, size_t& cub_bytes) { return (call); })) return rc_; \
    } while (0)

// Temporaries of a stretch of queued work: every block handed out stays alive as long as this object, which its owner lets die behind
// a synchronisation (or under a PoolHold).  As a scratch for CUB_TRY it is ONE block shared by the calls — they run one after the
// other on their stream —, replaced by a larger one when a call needs more.
struct Temps {
    std::vector<std::unique_ptr<DevBuf>> keep;
    DevBuf* scratch = nullptr;
    DevBuf* take(size_t bytes) {  // a block of its own; nullptr: out of memory
        auto b = std::make_unique<DevBuf>();
        if (b->alloc(bytes)) return nullptr;
        keep.push_back(std::move(b));
        return keep.back().get();
    }
    void* operator()(size_t bytes) {
        if (!scratch || scratch->bytes < bytes) scratch = take(bytes);
        return scratch ? scratch->p : nullptr;
    }
};
// Scratch for CUB_TRY in a buffer that outlives the call (`b` is reused when it is large enough): only where nothing queued still uses
// what `b` holds.
inline auto scratch_in(DevBuf& b) {
    return [&b](size_t bytes) -> void* { return ((b.p && b.bytes >= bytes) || !b.alloc(bytes)) ? b.p : nullptr; };
}
