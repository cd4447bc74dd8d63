// bmo_engine.hip — MI355X (gfx950) trace engine behind the C ABI of include/bmo.h.
//
// Execution model: wavefront tracing, bounce levels fused per wave.
//   * One launch of step_kernel / step_kernel_gauss advances every ACTIVE beam node by up to 32 (31) bounces
//     (tracing_step! + interact3d, System.jl:133-152).  Lane j works on record j of the
//     current step chunk; the segment log IS the sequence of step chunks (SoA planes), so a
//     bounce reads the 64 B it needs (pos, dir, n, hint) and writes intersection + next
//     segment once — SURVEY.md §8d's 184 B/bounce.  Inside a launch a beam that goes on writes
//     its next record in place (same slot of the next in-place chunk); every wave runs its
//     own level loop and notes how far it got (Chunk::wl).  A beam splitter met in the loop keeps
//     its transmitted child in the lane and pushes the reflected one to the next launch's chunk
//     (one reservation per wave).
//   * The scene tables (objects, shapes, triangles, n(lambda), candidate table) stay in global memory
//     and are read with SCALAR loads through constant-address-space pointers: the wave works on one
//     shape at a time, lanes that disagree on it take turns (bmo_lane.hpp "scalar scene access").
//     Rays stay in HBM as structure-of-arrays planes (coalesced 8 B/lane loads); LDS holds two
//     per-lane columns only (the union children's Lipschitz memory, the lane memory of tracing_step).
//   * Survivors of a launch's last fused level are compacted into the next chunk with a wave
//     ballot + prefix popcount and ONE atomic per workgroup.
//   * After the last step, nodes are put in the reference's order (bundle order x BFS order):
//     heap-index bitmaps per root for trees of up to 5 levels, a radix sort on (root, depth,
//     path) keys up to 26, level-by-level ranking beyond; detector hits are compacted in that
//     order (scan + gather) so the hit buffers equal the reference's push! order.
// No CPU fallback: every entry point that traces requires a HIP device.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <unistd.h>
#include <memory>
#include <mutex>
#include <string>
#include <map>
#include <vector>

#include "bmo_lane.hpp"
#include "bmo_scene_blob.hpp"  // the scene blob (LDS image): BlobHeader, view_of, the host-side builder

using namespace bmo;

namespace {

thread_local std::string g_err;
// The switches of the engine, all read from the environment by read_switches below and nowhere else (DESIGN.md §3 "Switches" is the
// table of them: when each is read, its default, what it selects, who sets it).  Three groups by WHEN the value counts:
struct Knobs {  // once per process (knobs())
    bool debug;          // BMO_DEBUG: phase and step log on stderr
    bool keep_kids;      // BMO_KEEP_KIDS=0: no kept reflected children (StepParams::pend / ::gkeep)
    int64_t thin_waves;  // BMO_THIN_WAVES=<n>: a launch of fewer than n waves spreads its records over more waves (plan_launch)
    bool lpt;            // BMO_LPT=0: no tile-order feedback (tile_order_feedback)
    int reverse;         // BMO_REVERSE=<0|1|2>: StepParams::reverse (-1: the default)
    bool pool_poison;    // BMO_POOL_POISON: every block DevBuf / HostBuf hand out is filled with POOL_POISON_WORD first (bmo_pool.inc.hpp)
};
struct SolveSwitches {  // at the start of every solve (run_trace): the tests change these between solves
    int fuse, fuse_gauss;     // BMO_FUSE / BMO_FUSE_GAUSS=<n>: at most n bounce levels per launch (unset: INT_MAX, what the kernels take)
    int64_t wide_min_waves;   // BMO_WIDE_MIN_WAVES=<n>: the 4-waves-per-SIMD build from n waves per launch (launch_step)
    bool force_sort_order;    // BMO_FORCE_SORT_ORDER: test hook, no tree is ordered by heap index (order_nodes)
    bool force_deep_order;    // BMO_FORCE_DEEP_ORDER: test hook, every tree is ordered level by level (order_nodes)
    bool gaps;                // BMO_GAPS: device idle time between two launches on stderr
    bool timeline;            // BMO_TIMELINE: wave timeline of every launch (developer builds with BMO_DEV_TIMELINE)
};
struct Switches {
    Knobs process;
    SolveSwitches solve;
    const char* root_order;  // at every upload: BMO_ROOT_ORDER = chord | mask | none (nullptr: unset, auto; root_order_wanted)
};
Switches read_switches() {
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    auto num = [](const char* name, long long unset) { return getenv(name) ? atoll(getenv(name)) : unset; };
    auto small = [](const char* name, int unset) { return getenv(name) ? atoi(getenv(name)) : unset; };
    static const Knobs process{set("BMO_DEBUG"), num("BMO_KEEP_KIDS", 1) != 0, num("BMO_THIN_WAVES", 0), num("BMO_LPT", 1) != 0, (int)num("BMO_REVERSE", -1),
                                set("BMO_POOL_POISON")};
    Switches s;
    s.process = process;  // (the first call's values: a solve does not pay for them again)
    s.solve = SolveSwitches{small("BMO_FUSE", INT_MAX), small("BMO_FUSE_GAUSS", INT_MAX), num("BMO_WIDE_MIN_WAVES", 4096), set("BMO_FORCE_SORT_ORDER"),
                            set("BMO_FORCE_DEEP_ORDER"), set("BMO_GAPS"), set("BMO_TIMELINE")};
    s.root_order = getenv("BMO_ROOT_ORDER");
    return s;
}
const Knobs& knobs() {  // (asked at every launch and DBG line: it keeps the group, read_switches would read the per-solve names again)
    static const Knobs k = read_switches().process;
    return k;
}
bool dbg_on() { return knobs().debug; }
#define DBG(...)                          \
    do {                                  \
        if (dbg_on()) {                   \
            fprintf(stderr, "[bmo] " __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            fflush(stderr);               \
        }                                 \
    } while (0)
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                                    \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            return fail(e_ == hipErrorOutOfMemory ? BMO_ERR_OOM : BMO_ERR_NO_DEVICE,                      \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                              \
        }                                                                                                \
    } while (0)

// ------------------------------------------------------------------ record layout
// double planes per record: ABI planes first (include/bmo.h), then accumulators
//   RAY:       0-6 px py pz dx dy dz n | 7-10 t nx ny nz | 11 opl_acc
//   POLARIZED: 0-10 as RAY | 11-16 Re/Im E0 | 17 opl_acc
// int planes: 0 node, 1 k, 2 hint_obj, 3 hint_shape, 4 obj, 5 shape, 6 flags
template <int KIND>
struct Layout;
template <>
struct Layout<BMO_BEAM_RAY> {
    static constexpr int ABI = 11, ND = 12, OPL = 11;
};
template <>
struct Layout<BMO_BEAM_POLARIZED> {
    static constexpr int ABI = 17, ND = 18, OPL = 17;
};
//   GAUSSIAN:  chief 0-10 | waist 11-21 | divergence 22-32 | 33 lenA 34 lenB 35 oplC 36 oplW 37 oplD
template <>
struct Layout<BMO_BEAM_GAUSSIAN> {
    static constexpr int ABI = 33, ND = 38, OPL = 35;
    static constexpr int RAY_STRIDE = 11;  // planes per sub-ray (chief, waist, divergence): ray r starts at plane RAY_STRIDE * r
    static constexpr int LEN_A = 33, LEN_B = 34, OPL_C = 35, OPL_W = 36, OPL_D = 37;
    // staging planes of a reflected child (StepParams::gstage, ::gkeep): its three rays without their hits, planes STAGE_STRIDE * r + c;
    // a kept child (gkeep) has three more planes behind them
    static constexpr int STAGE_STRIDE = 7, STAGE_PLANES = 3 * STAGE_STRIDE, KEEP_L0 = 21, KEEP_OPLC = 22, KEEP_FLAGS = 23, KEEP_PLANES = 24;
};
using LG = Layout<BMO_BEAM_GAUSSIAN>;
constexpr int NI = 7;
enum { I_NODE = 0, I_K = 1, I_HOBJ = 2, I_HSHAPE = 3, I_OBJ = 4, I_SHAPE = 5, I_FLAGS = 6 };
enum { F_DEAD = 1 };

struct Chunk {
    double* d;   // [ND][cap]
    int32_t* i;  // [NI][cap]
    int64_t cap;
    int64_t count;
    // In-place level `level` (1..) of a fused launch: the slots of wave w (64 consecutive slots) hold records or hole marks only if that
    // wave got as far as this level, wl[w] >= level; what lies beyond was never written.  wl == nullptr: every slot below count is a record.
    // A launch over few records spreads them thinly — wave w owns the 2^wl_shift consecutive slots from w << wl_shift (StepParams::lane_shift).
    const uint8_t* wl = nullptr;
    int32_t level = 0;
    int32_t wl_shift = 6;
};
// node id of record j of a chunk of the log, -1 where there is none (a beam that ended earlier, or a level its wave did not reach)
__device__ __forceinline__ int32_t chunk_node(const Chunk& c, int64_t j) {
    if (c.wl && c.level > (int32_t)c.wl[j >> c.wl_shift]) return -1;
    return c.i[I_NODE * c.cap + j];
}

// interact's sink for the ray that goes on (bmo_lane.hpp NextInOut): the seven slots of the lane memory
struct NextInLaneMem {
    const LaneMem& lm;
    __device__ void put(const d3& pos, const d3& dir, double n) const {
        lm.put3(0, pos);
        lm.put3(3, dir);
        lm.m[7 * lm.stride] = n;  // (slot 6 is tracing_step's plate mark)
    }
};

struct Counters {  // device-resident, one per trace
    // records written to the next chunk.  Two slots: step s accumulates into slot s & 1 and clears the other one for step s + 1
    // (the host has read it before launching step s), so no host->device reset sits between two launches.
    unsigned long long next_count[2];
    unsigned long long node_count;
    unsigned long long max_depth;  // deepest beam-tree level created so far (sizes the sort keys of the final ordering)
    unsigned long long overflow;
    unsigned long long max_level[2];  // deepest in-place level any wave of the launch reached (slots used like next_count's)
    unsigned long long inwave[2];     // reflected children pushed from inside the fused loops of the launch (slots used like next_count's)
    unsigned long long sweep_mixed;   // sweep launches: waves whose lanes did not all belong to one configuration (must stay 0)
};

struct NodeArrays {
    int32_t* root;
    int32_t* parent;
    int32_t* nseg;
    int32_t* status;
    int32_t* li;
    int32_t* hit_det;
    unsigned long long* key;  // depth<<32 | path: one bit per tree level, newest lowest (0 transmitted, 1 reflected), last 32 levels kept
    double* lambda;
    double* hit;  // [cap][9 * hit_sub]
    double* aux;  // [cap][4]: Gaussian l0 (length of parent chief), w0, Re(E0), Im(E0)
    int64_t cap;
    int32_t hit_sub;  // detector records per node: 1 (Ray / PolarizedRay), 3 (GaussianBeamlet: chief, waist, divergence)
    int32_t* old;     // retrace only: node of the previous solution this beam re-walks, -1 once it traces freshly
    // [roots] the heap indices (tree_bits below: 2^depth - 1 + path) of the nodes of every root's tree, one bit each, for trees of up to 5
    // levels: set where the nodes are made (init_roots_kernel, the step kernels' make_children) so that the final ordering needs no pass
    // over the nodes to collect them; nullptr when the scene has no beam splitter
    unsigned long long* tbits;
};

// Tables of the previous solution a retrace re-walks (System.jl:188-255), indexed by ITS node ids; all device pointers.
struct OldChunk {  // one chunk of the previous solution's segment log
    const double* d;
    int64_t cap;
};
struct OldSolution {
    const int32_t* nseg;         // stored rays per beam
    const int32_t* status;       // BMO_NODE_SPLIT <=> the beam has (two) children
    const int32_t* first_child;  // node id of the transmitted child; the reflected one follows
    const int32_t* rec_start;    // exclusive scan of nseg
    const int32_t* rec_obj;      // [rec_start[node] + k]: object of the stored intersection of ray k, -1 = none
    const double* aux;           // Gaussian: [node][4] = l0, w0, Re E0, Im E0
    // where the stored rays are: record k of beam `node` is slot (loc & 2^40 - 1) of chunk (loc >> 40), loc = rec_loc[rec_start[node] + k].
    // Two situations read stored RAYS, not only the stored objects: children the reference keeps although the re-walk of their parent
    // ended in a `nothing` interaction before the splitter (they start from their stored first ray, System.jl:232-240), and a beamlet
    // that splits before the end of its stored path (its children are sized with the stale tail attached, ThinBeamsplitter.jl:125).
    const int64_t* rec_loc;
    const OldChunk* chunks;
};
constexpr int OLD_LOC_SHIFT = 40;
// planes and slot of stored record k of beam `node` of the previous solution
template <class Old>  // (OldSolution, in a kernel's arguments or behind step_params_again)
__device__ __forceinline__ const double* old_record(Old& O, int32_t node, int32_t k, int64_t& cap, int64_t& slot) {
    const int64_t loc = O.rec_loc[(int64_t)O.rec_start[node] + k];
    const OldChunk c = O.chunks[loc >> OLD_LOC_SHIFT];
    cap = c.cap;
    slot = loc & (((int64_t)1 << OLD_LOC_SHIFT) - 1);
    return c.d;
}

// Sweeps (bmo_trace_sweep, DESIGN.md §3 "Sweeps"): the scene blob holds one configuration per `stride` bytes, all with the same header.
// Lane v of the grid works on slot map[v] of the launch's chunk (-1: idle lane); the map groups the slots by configuration and pads every
// configuration's run to whole waves, so every wave traces records of ONE configuration and reads that configuration's tables with the
// scalar loads of bmo_lane.hpp.  root_cfg[root]: configuration of every root beam (non-decreasing).
struct SweepLanes {
    const int32_t* map;
    const int32_t* root_cfg;
    uint64_t stride;
};

#if !defined(BMO_MAX_FUSE)
#define BMO_MAX_FUSE 32
#endif
constexpr int MAX_FUSE = BMO_MAX_FUSE;
struct StepParams {
    BlobHeader hdr;  // copy of the scene blob's header
    const char* blob;
    uint32_t blob_bytes;
    int32_t use_lds;
    Chunk cur, nxt;
    Chunk inner[MAX_FUSE - 1];   // in-place levels 1..n_fuse-1 of this launch (capacity >= cur.count, same slot numbering as cur); the GaussianBeamlet
                                 // kernels use one more, inner[n_fuse - 1], for the rays of the last fused level (step_kernel_gauss)
    int32_t n_fuse;   // bounces per launch, 1..MAX_FUSE
    Counters* ctr;
    unsigned long long* call_shards;  // 64 counters, 128 B apart: reference intersect3d call count (metric numerator)
    NodeArrays nodes;
    int32_t r_max;
    int32_t parity;   // step & 1: which next_count slot this launch fills
    // RETR kernels read `old`, SWEEP kernels (fresh solves only) `sweep`: the two share their room, so the kernel arguments of the other
    // kernels keep their layout
    union {
        OldSolution old;
        SweepLanes sweep;
    };
    double* gstage;      // GaussianBeamlet kernels: [21][gstage_cap] staging planes of the reflected child's rays (GaussRecDev)
    int64_t gstage_cap;
    uint8_t* wave_last;  // [waves of the launch]: the last in-place level each wave reached (nullptr: nobody will read the log)
    // Records per wave = 2^lane_shift (6: every lane has one).  A level of a wave takes as long as its slowest lane, and the launches of a
    // deep beam tree's tail have far fewer records than the device has lanes: spread over more waves (the upper lanes idle) a slow march
    // holds up 2^lane_shift - 1 neighbours instead of 63.  Record j lives in lane j & (2^lane_shift - 1) of wave j >> lane_shift.
    int32_t lane_shift;
    // Room in P.nxt (and in the node arrays) for beam-splitter children made INSIDE the fused loop: a splitting lane goes on with its transmitted
    // child in place and pushes the reflected one to the next launch, as long as the launch has pushed fewer than this many; after that a
    // split ends the wave's loop as it always did (block_alloc has room for two records per lane whatever happened before).
    int64_t inwave_cap;
    int64_t nodes0;  // beams (nodes) in existence when the launch starts
    // Beam kernels with in-loop splitters: the reflected child of a splitting lane waits in slot j of this chunk (capacity >= cur.count) while
    // the lane goes on with the transmitted child; when that beam ends — and the wave's loop goes on — the lane takes its kept child up
    // itself, in the same launch (depth first).  The launch that used to follow for the reflected children alone lasted as long as the
    // slowest single march among them (SURVEY 8(d)'s config-2 bundle: two grazing marches of ~1 000 evaluations in 10^6 children, 1.3 ms
    // of a 5.5 ms solve with the device idle); inside the first launch those chains run beside everybody else's work.  A lane keeps ONE
    // child: a second split while one waits pushes the new reflected child to P.nxt as before; children still waiting when the wave's
    // loop ends are compacted into P.nxt behind the survivors.  d == nullptr: off.
    Chunk pend;
    double* gkeep;  // GaussianBeamlet kernels: the kept reflected child of lane j, [24][gstage_cap]: its rays as in gstage, then l0, oplC, flags
    // Workgroup b of the grid works on tile (grid - 1 - b) instead of tile b: the LAST records of the chunk start first.  The hardware hands
    // out workgroups in index order, a launch lasts until its slowest wave is done, and the slow waves of a bundle are its edge rays —
    // grazing exits through lens barrels, marches of 500 - 1 000 evaluations that are one dependent chain of ~1 ms each; a disc source
    // (BeamGroups.jl:232-243: radius grows with the index) has them at the END of the bundle, and children are queued in the order their
    // parents finished, the slow ones last again.  Started first, those chains run beside the bulk of the launch instead of behind it.
    int32_t reverse;
    // Longest-processing-time-first, from feedback (first launch of a solve over a batch that has been solved before): workgroup b works on
    // tile tile_order[b], the tiles sorted by the time they took in the previous solve of this batch, slowest first — the hardware hands out
    // workgroups in index order and a launch ends when its slowest wave does.  tile_cost[tile]: this launch's time of every tile
    // (s_memrealtime ticks), written for the next solve.  Both nullptr: `reverse` decides.  Results do not depend on any of it.
    const int32_t* tile_order;
    uint32_t* tile_cost;
#if defined(BMO_DEV_TIMELINE)
    unsigned long long* tl;  // developer builds: [2 * wave] start, [2 * wave + 1] end of every wave (wall_clock64, 100 MHz)
#endif
};

// The launch parameters where they are used.  A step kernel's only argument is its StepParams, ~2 KB at offset 0 of the kernel-argument
// segment: constant-address-space memory the wave reads with scalar loads.  Read as `P.field`, every field the code BEHIND the marches
// wants (chunks, node arrays, counters: some forty pointers and sizes) is loaded once at the kernel's entry, and as the marches leave no
// scalar register free the values are parked in the lanes of vector registers for the whole kernel — 124 v_writelane in the headline
// kernel's prologue, several hundred v_readlane at the level boundaries, each a vector instruction of a kernel that is bound by vector
// issue.  step_params_again() hands out the address of the same arguments through an empty asm the optimiser cannot see through: the
// fields read through it are loaded where the statement stands, by scalar loads served by the scalar cache, and are dead again before
// the next march.  Called once per level at the loop head and once behind tracing_step; only what the marches themselves need (the
// SceneView) is read from `P` directly.  Nothing is copied: the struct is never addressed in scratch.
// PRECONDITION: the StepParams is the kernel's FIRST explicit argument (offset 0 of the segment) and the caller is inlined into that
// __global__ function — the address is the running kernel's argument segment, whatever kernel that is.  Both step kernels take the
// StepParams as their only argument (launch_step is their one launch site) and say so at their signatures.
// HELD = true gives the plain address of `P` instead, i.e. the form before: the sweep builds keep it (with the lanes-below mask and the
// thread index as they were, prefix_rank / step_tid below) — read again, seven of them needed 4 - 16 B MORE scratch per lane.
typedef const BMO_KONST StepParams KStepParams;
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ KStepParams* kernel_args_again() {
    KStepParams* q = (KStepParams*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    return q;
}
#else
__host__ __device__ inline KStepParams* kernel_args_again() { return nullptr; }  // (host pass of the kernels' bodies: never runs)
#endif
template <bool HELD>
__device__ __forceinline__ auto step_params_again(const StepParams& P) {
    if constexpr (HELD) return &P;
    else return kernel_args_again();
}
// a chunk of the launch as the HELD builds have it, a copy, where the others have its address in the arguments (both: c->cap, c->d, c->i)
struct HeldChunk {
    Chunk c;
    __device__ const Chunk* operator->() const { return &c; }
};

// Per-lane retrace context (shared by the Beam and the GaussianBeamlet step kernels; tests/emu walks the same rules)
struct RetraceLane {
    int32_t old = -1, old_n = 0, probe_obj = -1;
    bool probe = false, fresh_allowed = true, missed = false;
};
template <class Params>  // (const StepParams*, or what step_params_again hands out)
__device__ __forceinline__ RetraceLane retrace_lane(Params* P, int32_t node, int32_t k) {
    RetraceLane r;
    r.old = P->nodes.old[node];
    if (r.old >= 0) {
        r.old_n = P->old.nseg[r.old];
        r.probe_obj = P->old.rec_obj[(int64_t)P->old.rec_start[r.old] + k];
        r.fresh_allowed = k + 1 < P->r_max;
        r.probe = r.probe_obj >= 0;
        r.missed = !r.probe;  // a stored ray without intersection: cleanup, trace_system! goes on without a hint
    }
    return r;
}

__device__ inline int lane_id() { return (int)(threadIdx.x & 63); }
// lanes below this one that are set in `mask`
template <bool MBCNT = true>
__device__ inline int prefix_rank(unsigned long long mask) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (!MBCNT) return __popcll(mask & ((1ull << lane_id()) - 1ull));
    // (the count instruction made for it: the mask of the lanes below, a loop invariant, is not built — the step kernels held it in two
    //  registers, or 8 B of scratch, across their marches)
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
#else
    return __popcll(mask & ((1ull << lane_id()) - 1ull));
#endif
}


// Slot and configuration of this lane of a sweep launch (StepParams::sweep).  The configuration of the lane's record (node -> root ->
// root_cfg) is read by every lane, the first lane's value is made wave-uniform, and the wave checks that its lanes agree: a wave that mixes
// configurations traces nothing and is counted (Counters::sweep_mixed fails the solve with BMO_ERR_INTERNAL), never a wrong answer.
__device__ __forceinline__ int32_t sweep_lane(const StepParams& P, int64_t gwave, int64_t& j, bool& valid) {
    const int32_t s = P.sweep.map[(gwave << 6) + lane_id()];
    j = s;
    valid = s >= 0;
    int32_t lc = -1;
    if (valid) lc = P.sweep.root_cfg[P.nodes.root[P.cur.i[I_NODE * P.cur.cap + s]]];
    const unsigned long long on = __ballot(valid);
    int32_t c = __shfl(lc, on ? __ffsll((unsigned long long)on) - 1 : 0);
    c = BMO_UNIFORM(c < 0 ? 0 : c);
    if (!BMO_WAVE_ALL(!valid || lc == c)) {
        if (lane_id() == 0) atomicAdd(&P.ctr->sweep_mixed, 1ull);
        valid = false;
    }
    return c;
}

// Block-aggregated slot allocation.  A single address sustains only ~88 returning atomics/us (MI355X_MICROARCH.md
// "dequeue"): one atomic per wave = 16 K per 1 M-ray launch put a ~0.3 ms floor under every launch.  Here the 4 waves
// of a block publish their ballot counts in LDS, thread 0 issues ONE atomic per counter, and every wave derives its
// own offsets.  Block layout in the next chunk: [survivors of wave 0..3][child pairs of wave 0..3].
#ifndef BMO_BLOCK
// Lanes per workgroup of the step kernels (a multiple of 64, at most 256).  Round 4: ONE wave per workgroup.  A workgroup keeps its LDS and
// its place among a CU's resident workgroups until its LAST wave is done, and the waves of a ragged launch end far apart (one grazing march
// holds a wave for milliseconds): with four waves per workgroup the ragged config-2 bundle ran with a third to two thirds of the wave slots
// EMPTY in the middle of its launch although thousands of workgroups were waiting (profiles/r04_timeline_c2v.txt) — 9.3 ms per solve, 7.5 ms
// with one wave per workgroup; the coherent bundles pay 0.5 % for four times as many workgroups (c2 3.42 -> 3.44 ms, c5 8.12 -> 8.17 ms;
// profiles/r04_ab_scheduling.txt item 9).  The slot allocation below is per workgroup either way; with one wave its barriers compile away.
#define BMO_BLOCK 64
#endif
// Thread of its workgroup, for the step kernels (launched with BMO_BLOCK lanes per workgroup).  With one wave per workgroup the lane number says it
// all, and said so — the compiler does not take it from the launch bounds — the wave of the workgroup is the constant 0 and the wave of the
// grid a scalar, where they were per-lane values held (the wide kernels: spilled to scratch) across the marches.
// (HELD: threadIdx.x and blockDim.x as they come — the sweep builds, see step_params_again)
template <bool HELD = false>
__device__ __forceinline__ unsigned step_tid() { return (BMO_BLOCK == 64 && !HELD) ? (threadIdx.x & 63u) : threadIdx.x; }
template <bool HELD = false>
__device__ __forceinline__ unsigned step_block() { return HELD ? blockDim.x : (unsigned)BMO_BLOCK; }
struct SlotAlloc {
    unsigned long long surv_base, child_base, node_base;
    unsigned long long m_surv, m_split;
};
// PAIRS = false: the second channel counts single records that need no new nodes (reflected children a lane kept for itself and
// could not get to before its wave's loop ended, StepParams::pend): block layout [survivors of wave 0..3][kept children of wave 0..3].
template <bool PAIRS, bool HELD, class Params>
__device__ __forceinline__ SlotAlloc block_alloc(bool survive, bool split, uint32_t calls, Params* P, char* scratch, int level = 0) {
    uint32_t* w32 = reinterpret_cast<uint32_t*>(scratch);                         // [0..3] surv, [4..7] split, [8..11] calls, [12..15] level
    unsigned long long* w64 = reinterpret_cast<unsigned long long*>(scratch + 32);  // [0] base, [1] nbase
    SlotAlloc a;
    a.m_surv = __ballot(survive);
    a.m_split = __ballot(split);
    const int wave = (int)(step_tid<HELD>() >> 6);
    unsigned int c = calls;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if (lane_id() == 0) {
        w32[wave] = (uint32_t)__popcll(a.m_surv);
        w32[4 + wave] = (uint32_t)__popcll(a.m_split);
        w32[8 + wave] = c;
        w32[12 + wave] = (uint32_t)level;
    }
    __syncthreads();
    if (step_tid<HELD>() == 0) {
        uint32_t ts = 0, tp = 0, tc = 0, ml = 0;
        for (int w = 0; w < BMO_BLOCK / 64; ++w) {
            ts += w32[w];
            tp += w32[4 + w];
            tc += w32[8 + w];
            ml = w32[12 + w] > ml ? w32[12 + w] : ml;
        }
        if (ml) atomicMax(&P->ctr->max_level[P->parity], (unsigned long long)ml);
        unsigned long long b = 0, nb = 0;
        if (ts + tp) b = atomicAdd(&P->ctr->next_count[P->parity], (unsigned long long)(ts + (PAIRS ? 2 : 1) * tp));
        if (PAIRS && tp) nb = atomicAdd(&P->ctr->node_count, (unsigned long long)(2 * tp));
        if (tc) atomicAdd(&P->call_shards[(blockIdx.x & 63u) * 16u], (unsigned long long)tc);  // sharded, no return value
        w64[0] = b;
        w64[1] = nb;
    }
    __syncthreads();
    uint32_t ps = 0, pp = 0, ts = 0;
    for (int w = 0; w < BMO_BLOCK / 64; ++w) {
        if (w < wave) {
            ps += w32[w];
            pp += w32[4 + w];
        }
        ts += w32[w];
    }
    a.surv_base = w64[0] + ps;
    a.child_base = w64[0] + ts + (PAIRS ? 2ull : 1ull) * pp;
    a.node_base = w64[1] + 2ull * pp;
    return a;
}

// Which tile of the chunk workgroup b of the grid works on (StepParams::reverse): 0 tile b; 1 the tiles from the end; 2 from both ends
// towards the middle (b even: tile b / 2, b odd: tile grid - 1 - b / 2).
__device__ __forceinline__ unsigned tile_of_block(int mode, unsigned b, unsigned grid) {
    if (mode == 1) return grid - 1u - b;
    if (mode == 2) return (b & 1u) ? grid - 1u - (b >> 1) : (b >> 1);
    return b;
}
// Waves per SIMD a step-kernel variant is compiled for = its register budget (3: 168 VGPRs, 4: 128).  Round 3: with the scene tables read by scalar
// loads tracing_step is spill-free at 168 registers, and 3 waves/SIMD beat 2 by 12 % on C2, 17 % on the vignetted bundle and 28 % on C5
// (profiles/r03_ab_scalar_scene.txt).  Round 4, after the leaf-dispatch work: at 128 registers the Ray kernel of the plain-shapes level spills
// 60 - 92 B per lane (100 - 132 before the selection-form dual rules), all of it at bounce-level depth and none inside a march, and the fourth wave is worth more than that — on LARGE launches
// (profiles/r04_ab_scheduling.txt item 14: config 2 - 4 %, config 5 - 9 %, the ragged bundle - 9 %).  A launch of a few thousand waves is as long as its slowest
// marches, and those run slower with three neighbours on their SIMD than with two (2^18 rays of config 2: + 2 %), so the Ray kernels of that level are
// compiled twice and the launch picks by its size (`wide_min_waves` below: 4 096 waves, the device filled once at 4 per SIMD).  The other variants are compiled once, for the count that measured faster
// (tools/ext_times.py; the extended-shape levels and the polarized kernels spill 216 - 540 B at 128 registers, partly inside the normals' code).
// -DBMO_MIN_WAVES=n compiles every variant for n (A/B builds).
template <int KIND, int EXT, bool RETR>
constexpr int step_waves() {
#if defined(BMO_MIN_WAVES)
    return BMO_MIN_WAVES;
#else
    if (KIND == BMO_BEAM_POLARIZED && EXT == 0) return 4;  // three singlets, 2^18 PolarizedRays: fresh 0.317 against 0.341 ms, retrace 0.297 against 0.327
    if (RETR && EXT >= 2) return 4;                        // asphere objective: retrace 2.60 against 3.06 ms (Ray), 2.75 against 3.21 (PolarizedRay)
    return 3;
#endif
}
#ifndef BMO_MIN_WAVES_GAUSS
#define BMO_MIN_WAVES_GAUSS 3
#endif
// One launch advances every active beam by up to P.n_fuse bounces.  Bounce 0 reads its records from P.cur; a lane that goes
// on writes its next record IN PLACE (same slot j) into P.inner[b] and traces it in the same launch — no compaction, no host
// round trip, the ray stays in registers; lanes that ended leave an invalid record (node = -1) in the inner chunks.  The fused
// loop ends for a WAVE when one of its lanes splits (children need the slot allocation below) or when none goes on; the four waves
// of a workgroup run their loops independently and meet at the block-wide allocation.  Survivors of the last fused bounce and
// beam-splitter children are compacted into P.nxt as before.
// INW: beam splitters are handled inside the fused loop (the launches of a beam tree's tail: fewer launches, no launch waits for the
// slowest march of every generation); without it a split ends the wave's loop and both children wait for the next launch, which costs
// less register room — the large launches of the BASELINE configs run 2 - 7 % faster that way (profiles/r03_ab_inwave.txt).
// SWEEP (bmo_trace_sweep, fresh solves only): lane -> slot through StepParams::sweep, scene tables of the wave's configuration.
template <int KIND, int EXT, bool RETR, bool INW, int WAVES = step_waves<KIND, EXT, RETR>(), bool SWEEP = false>
__global__ __launch_bounds__(BMO_BLOCK, WAVES) void step_kernel(StepParams P) {  // (P: the ONLY argument — step_params_again reads the segment from offset 0)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    SceneView S = view_of((const char*)P.blob, &P.hdr);  // scene tables: global memory, scalar loads (bmo_lane.hpp)
    char* scratch = lds;
    if (blockIdx.x == 0 && step_tid<SWEEP>() == 0) {
        P.ctr->next_count[P.parity ^ 1] = 0;
        P.ctr->max_level[P.parity ^ 1] = 0;
        P.ctr->inwave[P.parity ^ 1] = 0;
    }
    using L = Layout<KIND>;
    const unsigned tile = P.tile_order ? (unsigned)P.tile_order[blockIdx.x] : tile_of_block(P.reverse, blockIdx.x, gridDim.x);
#if !defined(BMO_NO_TILE_COST)
    if (P.tile_cost && step_tid<SWEEP>() == 0) P.tile_cost[tile] = (uint32_t)wall_clock64();  // start stamp; turned into the tile's time at the end
#endif
    const int64_t gwave = ((int64_t)tile * step_block<SWEEP>() + step_tid<SWEEP>()) >> 6;  // wave of the grid
    int64_t sweep_j = 0;
    bool sweep_valid = false;
    if constexpr (SWEEP) {
        static_assert(!RETR, "sweeps are fresh solves");
        const int32_t cfg = sweep_lane(P, gwave, sweep_j, sweep_valid);
        S = view_of((const char*)P.blob + (uint64_t)cfg * P.sweep.stride, &P.hdr);
    }
    const int64_t j = SWEEP ? sweep_j : (gwave << P.lane_shift) + lane_id();
    const int64_t m = P.cur.count;
    const bool valid = SWEEP ? sweep_valid : (j < m && lane_id() < (1 << P.lane_shift));
#if defined(BMO_DEV_TIMELINE)
    if (P.tl && lane_id() == 0 && (gwave << P.lane_shift) < P.cur.count) P.tl[2 * gwave] = wall_clock64();
#endif

    // A lane carries nothing but `alive` from one fused bounce to the next: it writes its next record and reads it back at the
    // top of the next iteration (its own store, served by L1/L2) — keeping the ray in registers across the march instead costs
    // ~300 B/lane of scratch spills, and carrying only what the next march needs (position, direction, header) from the in-place store
    // to the loop top still costs 64 B of them and 0.8 % (round 2).
    bool alive = valid;
    uint32_t calls = 0;
    auto write_ray = [&](auto C, int64_t slot, const RayS& r, int32_t nd, int32_t kk, int32_t ho, int32_t hs, int32_t fl, double opl) {
        const int64_t ncap = C->cap;
        double* D = C->d;
        int32_t* I = C->i;
        D[0 * ncap + slot] = r.pos.x;
        D[1 * ncap + slot] = r.pos.y;
        D[2 * ncap + slot] = r.pos.z;
        D[3 * ncap + slot] = r.dir.x;
        D[4 * ncap + slot] = r.dir.y;
        D[5 * ncap + slot] = r.dir.z;
        D[6 * ncap + slot] = r.n;
        if (KIND == BMO_BEAM_POLARIZED)
            for (int c = 0; c < 3; ++c) {
                D[(11 + 2 * c) * ncap + slot] = r.E0[c].re;
                D[(12 + 2 * c) * ncap + slot] = r.E0[c].im;
            }
        D[L::OPL * ncap + slot] = opl;
        I[I_NODE * ncap + slot] = nd;
        I[I_K * ncap + slot] = kk;
        I[I_HOBJ * ncap + slot] = ho;
        I[I_HSHAPE * ncap + slot] = hs;
        I[I_FLAGS * ncap + slot] = fl;
    };

    int b = 0;  // fused bounce index: records of bounce b live in C = (b == 0 ? P.cur : P.inner[b - 1]) at slot j
    // What a lane that goes on in place takes to the top of the next level: the header of the record it has just written (registers — nothing
    // else is live there) and, in the lane memory, the ray's position and direction where interact's sink left them.  Reading the record
    // back from the chunk cost eleven loads from L2 per level, each at the head of the level's dependency chain.
    int32_t c_node = -1, c_k = 0, c_ho = -1, c_hs = -1, c_fl = 0;
    int32_t pend_node = -1;  // node of the reflected child this lane keeps for itself in P.pend[j] (StepParams::pend), -1: none
#if defined(BMO_DEV_TIMELINE)
    unsigned long long tk0 = 0, tk1 = 0, tk2 = 0, tk_last = wall_clock64();  // time before / in / after tracing_step, summed over the levels
#endif
    for (;;) {
        // (the launch's parameters are read where they are used: step_params_again)
        const auto Qh = step_params_again<SWEEP>(P);
        [[maybe_unused]] const HeldChunk held{SWEEP ? (b == 0 ? P.cur : P.inner[b - 1]) : Chunk{}};  // (the sweep builds: the level's chunk, held)
        // ---- the tracing step.  Only what it needs is read before it, and nothing the interaction needs is computed before it: the
        //      record addresses, node id and segment index are derived again behind it from a copy of the slot index the optimiser
        //      cannot see through (`jj`), so no address or header value of this level is held in a register (or spilled) across the
        //      marches — the ray's origin comes back from the lane memory of tracing_step, the hit's normal too.
        RetraceLane rt;
        int32_t node = -1, k = 0;  // (two registers across the marches; read again behind them they came back from HBM: the level's records
        d3 dir{0, 0, 0};           //  do not stay in L2 that long.  The direction is live in tracing_step anyway.)
        int32_t x_obj = -1, x_shape = -1;
        double x_t = kinf();
        bool traced = false;  // the lane ran a tracing step at this level (its record is not a pushed-but-never-traced one)
        const LaneMem lm{reinterpret_cast<double*>(scratch + 64) + BMO_CC_MAX * BMO_BLOCK + step_tid<SWEEP>(), BMO_BLOCK};
        const int32_t t_node = c_node, t_k = c_k, t_ho = c_ho, t_hs = c_hs, t_fl = c_fl;
        c_node = c_k = c_ho = c_hs = c_fl = 0;  // (dead from here to the next in-place write, in every lane: no register across the marches)
        if (alive) {
            const int64_t cap = SWEEP ? held->cap : Qh->cur.cap;  // (the input chunk: read at level 0 only)
            const double* D = SWEEP ? held->d : Qh->cur.d;
            const int32_t* I = SWEEP ? held->i : Qh->cur.i;
            int32_t flags = t_fl, ho = t_ho, hs = t_hs;
            node = t_node;
            k = t_k;
            if (b == 0) {  // (wave-uniform) the launch's input chunk
                flags = I[I_FLAGS * cap + j];
                ho = I[I_HOBJ * cap + j];
                hs = I[I_HSHAPE * cap + j];
                node = I[I_NODE * cap + j];
                k = I[I_K * cap + j];
            }
            if (RETR) {
                rt = retrace_lane(Qh, node, k);
                if (rt.old >= 0 && !rt.probe) ho = hs = -1;
            }
            traced = !((flags & F_DEAD) || (RETR && rt.old >= 0 && !rt.probe && !rt.fresh_allowed));  // else: pushed but never traced (System.jl:133)
            if (traced) {
                d3 pos;
                if (b == 0) {
                    pos = {D[0 * cap + j], D[1 * cap + j], D[2 * cap + j]};
                    dir = {D[3 * cap + j], D[4 * cap + j], D[5 * cap + j]};
                    // what the interaction will want behind the marches, into the lane memory with the same batch of loads (slots 7..10;
                    // from level 1 on they are there already: the beam's constants do not change along a lane, children included)
                    lm.m[7 * lm.stride] = D[6 * cap + j];
                    lm.m[8 * lm.stride] = D[L::OPL * cap + j];
                    lm.m[9 * lm.stride] = (double)Qh->nodes.li[node];
                    lm.m[10 * lm.stride] = Qh->nodes.lambda[node];
                } else {
                    pos = lm.get3(0);
                    dir = lm.get3(3);
                }
                // per-lane column of LDS behind the block_alloc scratch: Lipschitz memory of the union children (bmo_lane.hpp sdf_any)
                ChildCache cc{reinterpret_cast<double*>(scratch + 64) + step_tid<SWEEP>(), BMO_BLOCK, 0};
#if defined(BMO_DEV_TIMELINE)
                {
                    const unsigned long long t = wall_clock64();
                    tk0 += t - tk_last;
                    tk_last = t;
                }
#endif
                // (single-shape marches in the specialised loop, BMO_LEAF_MARCH: every variant but the PolarizedRay in-wave kernel of the
                //  plain-shapes level, which would hold 252 B of scratch with it instead of 240: DESIGN.md §4 "Round 6")
                constexpr bool LEAF = !(KIND == BMO_BEAM_POLARIZED && EXT == 0 && !RETR && INW && !SWEEP);
                // (the box cull, BMO_BOX_CULL.  Of the variants that hold the specialised march loops — the fresh kernels of the plain-shapes
                //  level — only the Ray kernel of the large launches runs it: with it the loops of the others take a scalar load per trip
                //  or eight lane operations they did not hold, so those stay on the parent's form: DESIGN.md §4 "Round 7")
                constexpr bool BOX = !(EXT == 0 && !RETR) || (KIND == BMO_BEAM_RAY && INW && WAVES == 4 && !SWEEP);
                const Hit X = tracing_step<EXT, RETR, LEAF, BOX>(S, pos, dir, ho, hs, calls, cc, lm, rt.probe, rt.probe_obj, rt.fresh_allowed, &rt.missed);
#if defined(BMO_DEV_TIMELINE)
                {
                    const unsigned long long t = wall_clock64();
                    tk1 += t - tk_last;
                    tk_last = t;
                }
#endif
                x_t = X.t;
                x_obj = X.obj;
                x_shape = X.shape;
            }
        }
        // ---- the interaction and the record of this level
        int64_t jj = j;
        asm volatile("" : "+v"(jj));
        const auto Q = step_params_again<SWEEP>(P);
        const auto C = [&] {  // the chunk of this level
            if constexpr (SWEEP) return held;
            else return b == 0 ? &Q->cur : &Q->inner[b - 1];
        }();
        bool survive = false, split = false, still = false, old_kids = false, stale_kids = false;
        double opl_next = 0.0, lambda = 0.0;
        int32_t li = 0;
        StepOut o;
        o.outcome = OUT_MISS;
        o.status = 0;
        o.hint_obj = o.hint_shape = -1;
        o.det_slot = -1;
        o.det = nullptr;
        // header of the record that follows a surviving bounce: r_max flag and hint, with the retrace overrides
        auto next_header = [&](int32_t& fl, int32_t& ho, int32_t& hs) {
            fl = (k + 2 < Q->r_max) ? 0 : F_DEAD;
            ho = o.hint_obj;
            hs = o.hint_shape;
            if (RETR && still) {
                if (k + 1 < rt.old_n) fl = 0;  // replace!: the next stored ray is re-walked whatever r_max says
                else ho = hs = -1;            // push!, then trace_system! starts over without a hint
            }
        };
        if (alive) {
            const int64_t cap = C->cap;
            double* D = C->d;
            int32_t* I = C->i;
            Hit X;
            X.t = x_t;
            X.obj = x_obj;
            X.shape = x_shape;
            X.n = {0, 0, 0};
            int status = 0;
            if (!traced) {
                status = BMO_NODE_RMAX;
            } else if (x_shape < 0) {
                status = (RETR && rt.old >= 0 && rt.missed && !rt.fresh_allowed) ? BMO_NODE_RMAX : BMO_NODE_MISS;
            } else {
                X.n = lm.get3(0);
                RayS ray;  // the interaction's share of the record
                ray.pos = lm.get3(3);
                ray.dir = dir;
                ray.n = lm.m[7 * lm.stride];
                if (KIND == BMO_BEAM_POLARIZED)
                    for (int c = 0; c < 3; ++c) ray.E0[c] = {D[(11 + 2 * c) * cap + jj], D[(12 + 2 * c) * cap + jj]};
                const double opl_acc = lm.m[8 * lm.stride];
                li = (int32_t)lm.m[9 * lm.stride];
                lambda = lm.m[10 * lm.stride];
                o.det = Q->nodes.hit + (int64_t)node * 9;  // a detector hit ends the beam: its record goes straight to the node's slot
                // (the ray that goes on is put into the lane memory — hit normal, origin and plate mark there are spent — as soon as a
                //  branch of the interaction has it, and comes back from there when its record is written: bmo_lane.hpp NextInOut)
                interact<KIND>(S, ray, X, li, lambda, opl_acc, o, NextInLaneMem{lm});
                status = o.status;
                if (o.outcome == OUT_CONTINUE) {
                    survive = true;
                    opl_next = opl_acc + X.t * ray.n;
                } else if (o.outcome == OUT_SPLIT) {
                    split = true;
                    status |= BMO_NODE_SPLIT | BMO_NODE_STOPPED;
                    opl_next = opl_acc + X.t * ray.n;
                } else {
                    status |= BMO_NODE_STOPPED;
                    if (RETR && rt.old >= 0 && rt.probe && !rt.missed && Q->old.first_child[rt.old] >= 0) {
                        // The re-walk ends here in a `nothing` interaction, before the splitter the stored beam ended on: the reference cuts the
                        // tail but KEEPS the children (cleanup_children stays false, System.jl:232-240); solve_system! then retraces each of them
                        // from its stored first ray (System.jl:446-458).  The two stored heads take the places a splitter's children have: the
                        // transmitted one in the lane memory (o.next for the field vector), the reflected one in o.refl.
                        stale_kids = true;
                        opl_next = opl_acc + X.t * ray.n;  // optical_path_length(parent): every ray of the cut beam up to this hit (Beam.jl:137-149)
                        const int32_t oc = Q->old.first_child[rt.old];
                        int64_t hc, hs;
                        const double* H = old_record(Q->old, oc, 0, hc, hs);
                        lm.put3(0, d3{H[0 * hc + hs], H[1 * hc + hs], H[2 * hc + hs]});
                        lm.put3(3, d3{H[3 * hc + hs], H[4 * hc + hs], H[5 * hc + hs]});
                        lm.m[7 * lm.stride] = H[6 * hc + hs];
                        if (KIND == BMO_BEAM_POLARIZED)
                            for (int c = 0; c < 3; ++c) o.next.E0[c] = {H[(11 + 2 * c) * hc + hs], H[(12 + 2 * c) * hc + hs]};
                        H = old_record(Q->old, oc + 1, 0, hc, hs);
                        o.refl.pos = d3{H[0 * hc + hs], H[1 * hc + hs], H[2 * hc + hs]};
                        o.refl.dir = d3{H[3 * hc + hs], H[4 * hc + hs], H[5 * hc + hs]};
                        o.refl.n = H[6 * hc + hs];
                        if (KIND == BMO_BEAM_POLARIZED)
                            for (int c = 0; c < 3; ++c) o.refl.E0[c] = {H[(11 + 2 * c) * hc + hs], H[(12 + 2 * c) * hc + hs]};
                    }
                }
            }
            // intersection part of this record
            D[7 * cap + jj] = X.t;
            D[8 * cap + jj] = X.n.x;
            D[9 * cap + jj] = X.n.y;
            D[10 * cap + jj] = X.n.z;
            I[I_OBJ * cap + jj] = X.obj;
            I[I_SHAPE * cap + jj] = X.shape;
            if (RETR) {
                still = rt.old >= 0 && rt.probe && !rt.missed;  // the stored path held at this ray
                old_kids = still && Q->old.first_child[rt.old] >= 0;  // (not the SPLIT status: kept stale children hang on a beam that did not split)
                if (stale_kids) {  // from here on like a splitter's children, but the beam did not split: no BMO_NODE_SPLIT
                    status |= BMO_NODE_RETRACE_STALE;
                    split = true;
                }
                if (rt.old >= 0 && !(survive && still && k + 1 < rt.old_n)) Q->nodes.old[node] = -1;
            }
            if (!survive) {  // node ends here
                Q->nodes.nseg[node] = k + 1;
                Q->nodes.status[node] = status;
                if (o.det_slot >= 0) Q->nodes.hit_det[node] = o.det_slot;
            }
        }
#if defined(BMO_DEV_TIMELINE)
        {
            const unsigned long long t = wall_clock64();
            tk2 += t - tk_last;
            tk_last = t;
        }
#endif
        const int64_t ncap = Q->nxt.cap;
        auto write_next = [&](int64_t slot, const RayS& r, int32_t nd, int32_t kk, int32_t ho, int32_t hs, int32_t fl, double opl) {
            if (slot >= ncap) {
                atomicAdd(&Q->ctr->overflow, 1ull);
                return;
            }
            write_ray(&Q->nxt, slot, r, nd, kk, ho, hs, fl, opl);
        };
        // the two children of a splitting lane: nodes cn (transmitted) and cn + 1 (reflected)
        auto make_children = [&](int64_t cn) {
            const unsigned long long pkey = Q->nodes.key[node];
            const unsigned long long depth = pkey >> 32, path = pkey & 0xFFFFFFFFull;
            const int32_t root = Q->nodes.root[node];
            atomicMax(&Q->ctr->max_depth, depth + 1ull);
            if (Q->nodes.tbits && depth < 5) atomicOr(&Q->nodes.tbits[root], 3ull << ((2ull << depth) - 1ull + (path << 1)));  // both children's heap indices
            for (int w = 0; w < 2; ++w) {
                const int64_t c = cn + w;
                Q->nodes.root[c] = root;
                Q->nodes.parent[c] = node;
                Q->nodes.nseg[c] = 1;
                Q->nodes.status[c] = 0;
                Q->nodes.li[c] = li;
                Q->nodes.lambda[c] = lambda;
                Q->nodes.hit_det[c] = -1;
                Q->nodes.key[c] = ((depth + 1) << 32) | (((path << 1) | (unsigned long long)w) & 0xFFFFFFFFull);
                if (RETR) Q->nodes.old[c] = old_kids ? Q->old.first_child[rt.old] + w : -1;  // children!: the stored child is re-walked
            }
        };
        const int32_t child_flags = ((RETR && old_kids) || 1 < Q->r_max) ? 0 : F_DEAD;
        auto next_ray = [&]() {
            RayS r = o.next;  // (E0 of a PolarizedRay stays where it is)
            r.pos = lm.get3(0);
            r.dir = lm.get3(3);
            r.n = lm.m[7 * lm.stride];
            return r;
        };
        bool go_on = b + 1 < Q->n_fuse;
        // wave-uniform decisions: every wave runs its own fused loop (no workgroup barrier per level: the four waves of a workgroup used to
        // wait for the slowest of them at every bounce); the workgroup meets again at block_alloc below.
        // Beam splitters first, wherever in the loop they are met: one reservation per wave — a run of node pairs and a run of slots in
        // P.nxt — and, while the launch has room for it (inwave_cap), the splitting lane goes on with its transmitted child in place and
        // only the reflected one waits for the next launch; otherwise both wait there and the wave's loop ends.
        const unsigned long long m_split = INW ? __ballot(split) : 0ull;
        bool kid_here = false;  // this lane goes on with its transmitted child
#if defined(BMO_NO_KEEP)
        const bool keep = false;
#else
        const bool keep = INW && Q->pend.d != nullptr;  // reflected children stay with their lane (StepParams::pend)
#endif
        if (!INW) {
            if (go_on) go_on = !__any(split ? 1 : 0);
        } else if (m_split) {
            const int ns = __popcll(m_split);
            // splitting lanes whose reflected child has to go to P.nxt at once: all of them without `keep`, else those that keep one already
            const unsigned long long m_push = keep ? (m_split & __ballot(pend_node >= 0)) : m_split;
            const int np = __popcll(m_push);
            unsigned long long r1 = 0, r2 = 0;
            // the node pairs first: their running count is also the number of in-loop splits of this launch so far (every node a launch of
            // this kernel makes is made here), which the launch's room bounds — one returning atomic instead of two in a row
            if (lane_id() == 0) r2 = atomicAdd(&Q->ctr->node_count, 2ull * ns);
            r2 = __shfl(r2, 0);
            if (go_on && (int64_t)((r2 - (unsigned long long)Q->nodes0) / 2ull + ns) > Q->inwave_cap) go_on = false;  // (kept child or not: the bound also sizes the node table)
            if (!go_on || np) {
                if (lane_id() == 0) r1 = atomicAdd(&Q->ctr->next_count[Q->parity], (unsigned long long)(go_on ? np : 2 * ns));
                r1 = __shfl(r1, 0);
            }
            if (split) {
                const int r = prefix_rank<!SWEEP>(m_split);
                const int64_t cn = (int64_t)r2 + 2 * r;
                if (cn + 1 < Q->nodes.cap) {
                    make_children(cn);
                    const auto T = [&] {  // (wave-uniform)
                        if constexpr (SWEEP) return HeldChunk{go_on ? P.inner[b] : P.nxt};
                        else return go_on ? &Q->inner[b] : &Q->nxt;
                    }();
                    const int64_t ts = go_on ? jj : (int64_t)r1 + 2 * r;
                    if (ts < T->cap) write_ray(T, ts, next_ray(), (int32_t)cn, 0, -1, -1, child_flags, opl_next);
                    else atomicAdd(&Q->ctr->overflow, 1ull);
                    c_node = (int32_t)cn;
                    c_k = 0;
                    c_ho = c_hs = -1;
                    c_fl = child_flags;
                    lm.m[8 * lm.stride] = opl_next;
                    if (go_on && keep && pend_node < 0) {  // the reflected child waits for this lane
                        write_ray(&Q->pend, jj, o.refl, (int32_t)(cn + 1), 0, -1, -1, child_flags, opl_next);
                        pend_node = (int32_t)(cn + 1);
                    } else {
                        write_next(go_on ? (int64_t)r1 + prefix_rank<!SWEEP>(m_push) : (int64_t)r1 + 2 * r + 1, o.refl, (int32_t)(cn + 1), 0, -1, -1, child_flags, opl_next);
                    }
                    kid_here = go_on;
                } else {
                    atomicAdd(&Q->ctr->overflow, 1ull);
                }
            }
        }
        // a lane whose beam ends here takes up the reflected child it kept, if the wave goes on
        const bool take_kept = INW && valid && alive && !survive && !kid_here && pend_node >= 0;
        if (go_on) go_on = __any((survive || kid_here || take_kept) ? 1 : 0) != 0;
        if (go_on) {
            // go on in place: the next record of a surviving lane is written to the same slot of the next inner chunk
            const auto N = [&] {
                if constexpr (SWEEP) return HeldChunk{P.inner[b]};
                else return &Q->inner[b];
            }();
            if (valid) {
                if (alive && survive) {
                    int32_t fl, ho, hs;
                    next_header(fl, ho, hs);
                    write_ray(N, jj, next_ray(), node, k + 1, ho, hs, fl, opl_next);
                    c_node = node;
                    c_k = k + 1;
                    c_ho = ho;
                    c_hs = hs;
                    c_fl = fl;
                    lm.m[8 * lm.stride] = opl_next;
                } else if (take_kept) {
                    // the kept child's first record moves into the log (this level, this slot); its ray goes where a lane that goes on in
                    // place expects it: position, direction, index and optical path in the lane memory, the header in registers
                    const int64_t pc = Q->pend.cap, nc = N->cap;
                    BMO_NOUNROLL
                    for (int q = 0; q < L::ND; ++q) N->d[q * nc + jj] = Q->pend.d[q * pc + jj];
                    c_fl = Q->pend.i[I_FLAGS * pc + jj];
                    N->i[I_NODE * nc + jj] = pend_node;
                    N->i[I_K * nc + jj] = 0;
                    N->i[I_HOBJ * nc + jj] = -1;
                    N->i[I_HSHAPE * nc + jj] = -1;
                    N->i[I_FLAGS * nc + jj] = c_fl;
                    lm.put3(0, d3{Q->pend.d[0 * pc + jj], Q->pend.d[1 * pc + jj], Q->pend.d[2 * pc + jj]});
                    lm.put3(3, d3{Q->pend.d[3 * pc + jj], Q->pend.d[4 * pc + jj], Q->pend.d[5 * pc + jj]});
                    lm.m[7 * lm.stride] = Q->pend.d[6 * pc + jj];
                    lm.m[8 * lm.stride] = Q->pend.d[L::OPL * pc + jj];
                    c_node = pend_node;
                    c_k = 0;
                    c_ho = c_hs = -1;
                    pend_node = -1;
                } else if (!kid_here) {
                    N->i[I_NODE * N->cap + jj] = -1;  // no record of this beam at this level
                    alive = false;
                }
            }
            b += 1;
            continue;
        }
        // ---- last fused bounce of this wave (kept inside the loop so that o.next / o.refl die here instead of staying live
        //      across the march of the next iteration): note how far the wave got — the in-place levels beyond are never written and
        //      never read (Chunk::wl) —, then compact into the next launch's chunk
        if constexpr (SWEEP) {  // (a wave's slots are not consecutive: the level is noted per slot, Chunk::wl_shift = 0)
            if (Q->wave_last && valid) Q->wave_last[j] = (uint8_t)b;
        } else if (Q->wave_last && lane_id() == 0) {
            Q->wave_last[gwave] = (uint8_t)b;
        }
#if defined(BMO_DEV_TIMELINE)
        if (Q->tl && lane_id() == 0 && (gwave << Q->lane_shift) < Q->cur.count) {  // (tail waves of the grid have no slot in the timeline)
            Q->tl[2 * gwave + 1] = wall_clock64();  // before the workgroup barrier of block_alloc
            const int64_t nw = (Q->cur.count + (1 << Q->lane_shift) - 1) >> Q->lane_shift;
            atomicAdd(&Q->tl[2 * nw + 0], tk0);
            atomicAdd(&Q->tl[2 * nw + 1], tk1);
            atomicAdd(&Q->tl[2 * nw + 2], tk2);
        }
#endif
        const SlotAlloc al = INW ? block_alloc<false, SWEEP>(survive, pend_node >= 0, calls, Q, scratch, b) : block_alloc<true, SWEEP>(survive, split, calls, Q, scratch, b);
        if (survive) {  // survivors first
            const int64_t slot = (int64_t)al.surv_base + prefix_rank<!SWEEP>(al.m_surv);
            int32_t fl, ho, hs;
            next_header(fl, ho, hs);
            write_next(slot, next_ray(), node, k + 1, ho, hs, fl, opl_next);
        }
        if (INW && pend_node >= 0) {  // then the reflected children their lanes did not get to: whole records, P.pend -> P.nxt
            const int64_t slot = (int64_t)al.child_base + prefix_rank<!SWEEP>(al.m_split);
            if (slot < ncap) {
                const int64_t pc = Q->pend.cap;
                BMO_NOUNROLL
                for (int q = 0; q < L::ND; ++q) Q->nxt.d[q * ncap + slot] = Q->pend.d[q * pc + jj];
                BMO_NOUNROLL
                for (int q = 0; q < NI; ++q) Q->nxt.i[q * ncap + slot] = Q->pend.i[q * pc + jj];
            } else {
                atomicAdd(&Q->ctr->overflow, 1ull);
            }
        }
#if !defined(BMO_NO_TILE_COST)
        if (Q->tile_cost && step_tid<SWEEP>() == 0) Q->tile_cost[tile] = (uint32_t)wall_clock64() - Q->tile_cost[tile];  // (behind block_alloc's barrier: all four waves are done)
#endif
        if (!INW && split) {  // then 2 children per splitting lane
            const int r = prefix_rank<!SWEEP>(al.m_split);
            const int64_t slot = (int64_t)al.child_base + 2 * r;
            const int64_t cn = (int64_t)al.node_base + 2 * r;
            if (cn + 1 < Q->nodes.cap) {
                make_children(cn);
                write_next(slot, next_ray(), (int32_t)cn, 0, -1, -1, child_flags, opl_next);
                write_next(slot + 1, o.refl, (int32_t)(cn + 1), 0, -1, -1, child_flags, opl_next);
            } else {
                atomicAdd(&Q->ctr->overflow, 1ull);
            }
        }
        return;
    }
}


// ------------------------------------------------------------------ GaussianBeamlet step (System.jl:274-318)
// The beamlet record of lane j as gauss_step_rec sees it: rays come out of the chunk when a march starts, hits go back into it when
// the march ends (they are part of the log anyway), the accumulators are read after the marches.
struct GaussRecDev {
    double* D;
    const int32_t* I;
    const NodeArrays& nodes;
    int64_t cap, j;
    int32_t node;
    double* N;     // the next level's record planes (same slot j): the rays the step produces for the beamlet that goes on are written
    int64_t ncap;  // straight into their record, planes RAY_STRIDE r + c
    double* G;     // staging of the reflected child's rays: [STAGE_PLANES][gcap], planes STAGE_STRIDE r + c
    int64_t gcap;
    // wavelength index and wavelength of the beamlet: constant along a lane (children included), carried in the lane memory from the level
    // that loaded them — the node tables are indexed by beam, and with the roots in coherence order neighbouring lanes hold beams far apart:
    // six scattered reads per lane and level were 1.5 GB of the Gaussian kernel's HBM reads per config-3 solve
    int32_t li;
    double lambda;
    __device__ void put_next(int r, const RayS& x) const {
        const int64_t b = LG::RAY_STRIDE * (int64_t)r;
        N[(b + 0) * ncap + j] = x.pos.x;
        N[(b + 1) * ncap + j] = x.pos.y;
        N[(b + 2) * ncap + j] = x.pos.z;
        N[(b + 3) * ncap + j] = x.dir.x;
        N[(b + 4) * ncap + j] = x.dir.y;
        N[(b + 5) * ncap + j] = x.dir.z;
        N[(b + 6) * ncap + j] = x.n;
    }
    __device__ void put_refl(int r, const RayS& x) const {
        const int64_t b = LG::STAGE_STRIDE * (int64_t)r;
        G[(b + 0) * gcap + j] = x.pos.x;
        G[(b + 1) * gcap + j] = x.pos.y;
        G[(b + 2) * gcap + j] = x.pos.z;
        G[(b + 3) * gcap + j] = x.dir.x;
        G[(b + 4) * gcap + j] = x.dir.y;
        G[(b + 5) * gcap + j] = x.dir.z;
        G[(b + 6) * gcap + j] = x.n;
    }
    __device__ RayS ray(int r) const {
        const int64_t b = LG::RAY_STRIDE * (int64_t)r;
        RayS x;
        x.pos = {D[(b + 0) * cap + j], D[(b + 1) * cap + j], D[(b + 2) * cap + j]};
        x.dir = {D[(b + 3) * cap + j], D[(b + 4) * cap + j], D[(b + 5) * cap + j]};
        x.n = D[(b + 6) * cap + j];
        return x;
    }
    __device__ void put_hit(int r, const Hit& X) const {
        const int64_t b = LG::RAY_STRIDE * (int64_t)r;
        D[(b + 7) * cap + j] = X.t;
        D[(b + 8) * cap + j] = X.n.x;
        D[(b + 9) * cap + j] = X.n.y;
        D[(b + 10) * cap + j] = X.n.z;
    }
    __device__ Hit hit(int r) const {
        const int64_t b = LG::RAY_STRIDE * (int64_t)r;
        Hit X;
        X.t = D[(b + 7) * cap + j];
        X.n = {D[(b + 8) * cap + j], D[(b + 9) * cap + j], D[(b + 10) * cap + j]};
        X.obj = X.shape = -1;
        return X;
    }
    __device__ void clear_hits() const {
        const Hit X = no_hit();
        put_hit(0, X);
        put_hit(1, X);
        put_hit(2, X);
    }
    __device__ int32_t hint_obj() const { return I[I_HOBJ * cap + j]; }
    __device__ int32_t hint_shape() const { return I[I_HSHAPE * cap + j]; }
    __device__ GaussAcc acc() const {
        GaussAcc a;
        a.lenA = D[LG::LEN_A * cap + j];
        a.lenB = D[LG::LEN_B * cap + j];
        a.oplC = D[LG::OPL_C * cap + j];
        a.oplW = D[LG::OPL_W * cap + j];
        a.oplD = D[LG::OPL_D * cap + j];
        a.li = li;
        a.lambda = lambda;
        a.l0 = a.w0 = 0.0;  // (the splitter branch takes l0, w0, E0 from load(); nothing else reads them)
        a.E0 = {0.0, 0.0};
        return a;
    }
    __device__ GaussIn load() const {
        GaussIn g;
        g.c = ray(0);
        g.w = ray(1);
        g.d = ray(2);
        g.hint_obj = g.hint_shape = -1;  // consumed before the marches
        g.lenA = D[LG::LEN_A * cap + j];
        g.lenB = D[LG::LEN_B * cap + j];
        g.oplC = D[LG::OPL_C * cap + j];
        g.oplW = D[LG::OPL_W * cap + j];
        g.oplD = D[LG::OPL_D * cap + j];
        g.li = li;
        g.lambda = lambda;
        g.l0 = nodes.aux[(int64_t)node * 4 + 0];
        g.w0 = nodes.aux[(int64_t)node * 4 + 1];
        g.E0 = {nodes.aux[(int64_t)node * 4 + 2], nodes.aux[(int64_t)node * 4 + 3]};
        return g;
    }
};
// retrace: the stored rays behind the one a re-walking beamlet is at (bmo_lane.hpp gauss_step_rec `tail`), read from the previous
// solution's log
struct GaussTailDev {
    const OldSolution& O;
    int32_t old, k, old_n;
    __device__ int more() const { return old >= 0 ? old_n - (k + 1) : 0; }
    __device__ double t(int q) const {
        int64_t c, s;
        const double* D = old_record(O, old, k + 1 + q, c, s);
        return D[7 * c + s];
    }
    __device__ RayS ray(int q, int r) const {
        int64_t c, s;
        const double* D = old_record(O, old, k + 1 + q, c, s);
        const int64_t b = LG::RAY_STRIDE * (int64_t)r;
        RayS x;
        x.pos = {D[(b + 0) * c + s], D[(b + 1) * c + s], D[(b + 2) * c + s]};
        x.dir = {D[(b + 3) * c + s], D[(b + 4) * c + s], D[(b + 5) * c + s]};
        x.n = D[(b + 6) * c + s];
        return x;
    }
};
// retrace: a beamlet that re-walks its stored path without a probe starts without a hint
struct GaussRecDevNoHint : GaussRecDev {
    __device__ int32_t hint_obj() const { return -1; }
    __device__ int32_t hint_shape() const { return -1; }
};

// One launch advances every active beamlet by up to P.n_fuse bounces, like step_kernel: level b reads its records from C = (b == 0 ? P.cur :
// P.inner[b - 1]) at slot j and writes the rays of the beamlet that goes on IN PLACE into P.inner[b] at the same slot, as gauss_step_rec
// produces them (no staging copy, no compaction between the levels; P.inner has n_fuse entries here — the last one only holds the rays of
// the last fused level until they are compacted into P.nxt).  Beam splitters are handled in the loop: the transmitted child goes on in
// place, the reflected child's rays wait in the staging planes and are pushed to P.nxt (StepParams::inwave_cap).
template <int EXT, bool RETR, bool SWEEP = false>
__global__ __launch_bounds__(BMO_BLOCK, BMO_MIN_WAVES_GAUSS) void step_kernel_gauss(StepParams P) {  // (P: the ONLY argument — step_params_again reads the segment from offset 0)
    extern __shared__ __attribute__((aligned(16))) char lds[];
    SceneView S = view_of((const char*)P.blob, &P.hdr);  // scene tables: global memory, scalar loads (bmo_lane.hpp)
    char* scratch = lds;
    if (blockIdx.x == 0 && step_tid<SWEEP>() == 0) {
        P.ctr->next_count[P.parity ^ 1] = 0;
        P.ctr->max_level[P.parity ^ 1] = 0;
        P.ctr->inwave[P.parity ^ 1] = 0;
    }
    const unsigned tile = P.tile_order ? (unsigned)P.tile_order[blockIdx.x] : tile_of_block(P.reverse, blockIdx.x, gridDim.x);
#if !defined(BMO_NO_TILE_COST)
    if (P.tile_cost && step_tid<SWEEP>() == 0) P.tile_cost[tile] = (uint32_t)wall_clock64();  // start stamp; turned into the tile's time at the end
#endif
    const int64_t gwave = ((int64_t)tile * step_block<SWEEP>() + step_tid<SWEEP>()) >> 6;  // wave of the grid
    int64_t sweep_j = 0;
    bool sweep_valid = false;
    if constexpr (SWEEP) {
        static_assert(!RETR, "sweeps are fresh solves");
        const int32_t cfg = sweep_lane(P, gwave, sweep_j, sweep_valid);
        S = view_of((const char*)P.blob + (uint64_t)cfg * P.sweep.stride, &P.hdr);
    }
    const int64_t j = SWEEP ? sweep_j : (gwave << P.lane_shift) + lane_id();
    const int64_t m = P.cur.count;
    const bool valid = SWEEP ? sweep_valid : (j < m && lane_id() < (1 << P.lane_shift));
    bool alive = valid;
    uint32_t calls = 0;
    int32_t pend_node = -1;  // node of the reflected child this lane keeps for itself in P.gkeep (StepParams::pend), -1: none
    int b = 0;
    for (;;) {
        // (this level's chunk and the next one's come from `P` itself and are held: gauss_step_rec reads and writes the record through `rec`
        //  before, between and after its three marches, so their addresses are wanted all through the step; only what the code BEHIND the
        //  step wants — node arrays, counters, `nxt`, the kept children, the next chunk once more as Nq — is read again there)
        const Chunk C = b == 0 ? P.cur : P.inner[b - 1];
        const Chunk N = P.inner[b];
        const int64_t cap = C.cap;
        bool survive = false, split = false;
        int32_t node = -1, k = 0;
        GaussOut o;
        o.outcome = OUT_MISS;
        RetraceLane rt;
        bool still = false, old_kids = false;
        if (alive) {
            double* D = C.d;
            int32_t* I = C.i;
            node = I[I_NODE * cap + j];
            k = I[I_K * cap + j];
            const int32_t flags = I[I_FLAGS * cap + j];
            int status = 0;
            o.hit_obj = o.hit_shape = -1;
            o.det_slot = -1;
            o.det = P.nodes.hit + (int64_t)node * 27;  // a detector hit ends the beamlet: its records go straight to the node's slot
            bool no_hint = false;
            if (RETR) {
                rt = retrace_lane(&P, node, k);
                no_hint = rt.old >= 0 && !rt.probe;
            }
            // (lane memory slots 9, 10: wavelength index and wavelength; loaded where the lane's first record of this launch is read)
            const LaneMem lmw{reinterpret_cast<double*>(scratch + 64) + BMO_CC_MAX * BMO_BLOCK + step_tid<SWEEP>(), BMO_BLOCK};
            if (b == 0) {
                lmw.m[9 * lmw.stride] = (double)P.nodes.li[node];
                lmw.m[10 * lmw.stride] = P.nodes.lambda[node];
            }
            GaussRecDev rec{D, I, P.nodes, cap, j, node, N.d, N.cap, P.gstage, P.gstage_cap, (int32_t)lmw.m[9 * lmw.stride], lmw.m[10 * lmw.stride]};
            if ((flags & F_DEAD) || (RETR && rt.old >= 0 && !rt.probe && !rt.fresh_allowed)) {
                status = BMO_NODE_RMAX;
                rec.clear_hits();
            } else {
                ChildCache cc{reinterpret_cast<double*>(scratch + 64) + step_tid<SWEEP>(), BMO_BLOCK, 0};
                const LaneMem lm{reinterpret_cast<double*>(scratch + 64) + BMO_CC_MAX * BMO_BLOCK + step_tid<SWEEP>(), BMO_BLOCK};
                if (RETR && no_hint) {
                    GaussRecDevNoHint rn{{D, I, P.nodes, cap, j, node, N.d, N.cap, P.gstage, P.gstage_cap, rec.li, rec.lambda}};
                    gauss_step_rec<EXT, RETR>(S, rn, o, calls, cc, lm, rt.probe, rt.probe_obj, rt.fresh_allowed, &rt.missed);
                } else if (RETR) {
                    const GaussTailDev tail{P.old, rt.old, k, rt.old_n};
                    gauss_step_rec<EXT, RETR, GaussRecDev, GaussTailDev>(S, rec, o, calls, cc, lm, rt.probe, rt.probe_obj, rt.fresh_allowed, &rt.missed, tail);
                } else {
                    gauss_step_rec<EXT, RETR>(S, rec, o, calls, cc, lm, rt.probe, rt.probe_obj, rt.fresh_allowed, &rt.missed);
                }
                status = o.status;
                if (o.outcome == OUT_CONTINUE) survive = true;
                else if (o.outcome == OUT_SPLIT) {
                    split = true;
                    status |= BMO_NODE_SPLIT | BMO_NODE_STOPPED;
                } else if (o.outcome == OUT_STOP) status |= BMO_NODE_STOPPED;
            }
            // (behind the marches the launch's parameters are read again where they are used: step_params_again)
            const auto Qa = step_params_again<SWEEP>(P);
            I[I_OBJ * cap + j] = o.hit_obj;
            I[I_SHAPE * cap + j] = o.hit_shape;
            if (RETR) {
                still = rt.old >= 0 && rt.probe && !rt.missed;
                old_kids = still && Qa->old.first_child[rt.old] >= 0;  // (not the SPLIT status: kept stale children hang on a beamlet that did not split)
                if (!survive && old_kids && !split && !(flags & F_DEAD)) {
                    // The re-walk ends in a `nothing` interaction before the splitter the stored beamlet ended on: the reference keeps the children
                    // (System.jl:393-400) and retraces each from its stored first rays.  They take a splitter's children's places: the transmitted
                    // one's rays in the next level's record, the reflected one's in the staging planes; w0 and E0 stay the stored ones.
                    status |= BMO_NODE_RETRACE_STALE;
                    const int32_t oc = Qa->old.first_child[rt.old];
                    BMO_NOUNROLL
                    for (int w = 0; w < 2; ++w) {
                        int64_t hc, hs;
                        const double* H = old_record(Qa->old, oc + w, 0, hc, hs);
                        BMO_NOUNROLL
                        for (int r = 0; r < 3; ++r) {
                            const int64_t b11 = LG::RAY_STRIDE * (int64_t)r;
                            RayS x;
                            x.pos = {H[(b11 + 0) * hc + hs], H[(b11 + 1) * hc + hs], H[(b11 + 2) * hc + hs]};
                            x.dir = {H[(b11 + 3) * hc + hs], H[(b11 + 4) * hc + hs], H[(b11 + 5) * hc + hs]};
                            x.n = H[(b11 + 6) * hc + hs];
                            if (w == 0) rec.put_next(r, x);
                            else rec.put_refl(r, x);
                        }
                    }
                    o.child_l0 = o.lenA + Qa->nodes.aux[(int64_t)node * 4 + 0];  // length(parent chief): its rays up to this hit + its own parents (Beam.jl:125-130)
                    o.child_w0 = Qa->old.aux[(int64_t)oc * 4 + 1];
                    o.Et = {Qa->old.aux[(int64_t)oc * 4 + 2], Qa->old.aux[(int64_t)oc * 4 + 3]};
                    o.Er = {Qa->old.aux[(int64_t)(oc + 1) * 4 + 2], Qa->old.aux[(int64_t)(oc + 1) * 4 + 3]};
                    split = true;  // from here on like a splitter's children, but the beamlet did not split: no BMO_NODE_SPLIT
                }
                // a split before the end of the stored path: the reference sizes the children (w0, E0) with the stale tail still attached
                // to the beamlet (gauss_parameters(gauss, length(gauss)), ThinBeamsplitter.jl:125) — gauss_step_rec's `tail`; the flag stays as a note
                if ((status & BMO_NODE_SPLIT) && still && k + 1 < rt.old_n) status |= BMO_NODE_RETRACE_STALE;
                if (rt.old >= 0 && !(survive && still && k + 1 < rt.old_n)) Qa->nodes.old[node] = -1;
            }
            if (!survive) {
                Qa->nodes.nseg[node] = k + 1;
                Qa->nodes.status[node] = status;
                if (o.det_slot >= 0 && !(flags & F_DEAD)) Qa->nodes.hit_det[node] = o.det_slot;
            }
        }
        const auto Q = step_params_again<SWEEP>(P);
        const auto Nq = &Q->inner[b];  // the next level's record, same slot
        const int64_t ncap = Q->nxt.cap;
        // (measured twice, profiles/r04_ab_scheduling.txt items 5 and 11: while the leaves' dispatch still cost this kernel 196 B of scratch the kept
        //  child made it 228 B and config 3 2 % slower, 10.56 against 10.34 ms; with the pinned dispatch — 140 B, 164 with the kept child — it is
        //  2 % FASTER, 9.41 against 9.62 ms, and one launch per solve.  -DBMO_NO_GAUSS_KEEP compiles it out.)
#if defined(BMO_NO_GAUSS_KEEP)
        const bool keep = false;
#else
        const bool keep = Q->gkeep != nullptr;
#endif
        // accumulators and header of a record whose rays are in place already
        auto write_tail = [&](auto T, int64_t slot, int32_t nd, int32_t kk, int32_t ho, int32_t hs, int32_t fl, double lenA, double lenB, double oplC,
                              double oplW, double oplD) {
            const int64_t tcap = T->cap;
            double* D = T->d;
            int32_t* I = T->i;
            D[LG::LEN_A * tcap + slot] = lenA;
            D[LG::LEN_B * tcap + slot] = lenB;
            D[LG::OPL_C * tcap + slot] = oplC;
            D[LG::OPL_W * tcap + slot] = oplW;
            D[LG::OPL_D * tcap + slot] = oplD;
            I[I_NODE * tcap + slot] = nd;
            I[I_K * tcap + slot] = kk;
            I[I_HOBJ * tcap + slot] = ho;
            I[I_HSHAPE * tcap + slot] = hs;
            I[I_FLAGS * tcap + slot] = fl;
        };
        // a whole record in P.nxt: rays from `src` (plane r * rstride + c of capacity scap, at slot j), then accumulators and header
        auto write_next = [&](int64_t slot, const double* src, int64_t scap, int rstride, int32_t nd, int32_t kk, int32_t ho, int32_t hs, int32_t fl, double lenA,
                              double lenB, double oplC, double oplW, double oplD) {
            if (slot >= ncap) {
                atomicAdd(&Q->ctr->overflow, 1ull);
                return;
            }
            double* D = Q->nxt.d;
            BMO_NOUNROLL
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 7; ++c) D[(LG::RAY_STRIDE * r + c) * ncap + slot] = src[(int64_t)(rstride * r + c) * scap + j];
            write_tail(&Q->nxt, slot, nd, kk, ho, hs, fl, lenA, lenB, oplC, oplW, oplD);
        };
        // header of the record that follows a surviving bounce
        auto next_header = [&](int32_t& fl, int32_t& ho, int32_t& hs) {
            fl = (k + 2 < Q->r_max) ? 0 : F_DEAD;
            ho = o.hint_obj;
            hs = o.hint_shape;
            if (RETR && still) {
                if (k + 1 < rt.old_n) fl = 0;
                else ho = hs = -1;
            }
        };
        bool go_on = b + 1 < Q->n_fuse;
        // beam splitters, wherever in the loop they are met (see step_kernel): one reservation per wave
        const unsigned long long m_split = __ballot(split);
        bool kid_here = false;
        if (m_split) {
            const int ns = __popcll(m_split);
            const unsigned long long m_push = keep ? (m_split & __ballot(pend_node >= 0)) : m_split;  // reflected children that go to P.nxt at once
            const int np = __popcll(m_push);
            unsigned long long r1 = 0, r2 = 0;
            if (lane_id() == 0) r2 = atomicAdd(&Q->ctr->node_count, 2ull * ns);  // (also counts the launch's in-loop splits: see step_kernel)
            r2 = __shfl(r2, 0);
            if (go_on && (int64_t)((r2 - (unsigned long long)Q->nodes0) / 2ull + ns) > Q->inwave_cap) go_on = false;
            if (!go_on || np) {
                if (lane_id() == 0) r1 = atomicAdd(&Q->ctr->next_count[Q->parity], (unsigned long long)(go_on ? np : 2 * ns));
                r1 = __shfl(r1, 0);
            }
            if (split) {
                const int r = prefix_rank<!SWEEP>(m_split);
                const int64_t cn = (int64_t)r2 + 2 * r;
                if (cn + 1 < Q->nodes.cap) {
                    const unsigned long long pkey = Q->nodes.key[node];
                    const unsigned long long depth = pkey >> 32, path = pkey & 0xFFFFFFFFull;
                    const int32_t root = Q->nodes.root[node];
                    atomicMax(&Q->ctr->max_depth, depth + 1ull);
                    if (Q->nodes.tbits && depth < 5) atomicOr(&Q->nodes.tbits[root], 3ull << ((2ull << depth) - 1ull + (path << 1)));
                    for (int w = 0; w < 2; ++w) {
                        const int64_t c = cn + w;
                        Q->nodes.root[c] = root;
                        Q->nodes.parent[c] = node;
                        Q->nodes.nseg[c] = 1;
                        Q->nodes.status[c] = 0;
                        Q->nodes.li[c] = Q->nodes.li[node];
                        Q->nodes.lambda[c] = Q->nodes.lambda[node];
                        Q->nodes.hit_det[c] = -1;
                        Q->nodes.key[c] = ((depth + 1) << 32) | (((path << 1) | (unsigned long long)w) & 0xFFFFFFFFull);
                        Q->nodes.aux[c * 4 + 0] = o.child_l0;
                        Q->nodes.aux[c * 4 + 1] = o.child_w0;
                        Q->nodes.aux[c * 4 + 2] = w == 0 ? o.Et.re : o.Er.re;
                        Q->nodes.aux[c * 4 + 3] = w == 0 ? o.Et.im : o.Er.im;
                        if (RETR) {
                            const int32_t oc = old_kids ? Q->old.first_child[rt.old] + w : -1;
                            Q->nodes.old[c] = oc;
                            if (oc >= 0) Q->nodes.aux[c * 4 + 1] = Q->old.aux[(int64_t)oc * 4 + 1];  // _modify_beam_head! keeps the stored w0 (Gaussian.jl:154-161)
                        }
                    }
                    const int32_t fl = ((RETR && old_kids) || 1 < Q->r_max) ? 0 : F_DEAD;
                    // children: chief inherits the parent chain (parent! Gaussian.jl:113-117); waist/div beams have no parent
                    if (go_on) write_tail(Nq, j, (int32_t)cn, 0, -1, -1, fl, 0.0, o.child_l0, o.oplC, 0.0, 0.0);  // (its rays are in place)
                    else write_next((int64_t)r1 + 2 * r, Nq->d, Nq->cap, LG::RAY_STRIDE, (int32_t)cn, 0, -1, -1, fl, 0.0, o.child_l0, o.oplC, 0.0, 0.0);
                    if (go_on && keep && pend_node < 0) {  // the reflected child waits for this lane (the staging planes serve the next split)
                        const int64_t gc = Q->gstage_cap;
                        BMO_NOUNROLL
                        for (int q = 0; q < LG::STAGE_PLANES; ++q) Q->gkeep[q * gc + j] = Q->gstage[q * gc + j];
                        Q->gkeep[LG::KEEP_L0 * gc + j] = o.child_l0;
                        Q->gkeep[LG::KEEP_OPLC * gc + j] = o.oplC;
                        Q->gkeep[LG::KEEP_FLAGS * gc + j] = (double)fl;
                        pend_node = (int32_t)(cn + 1);
                    } else {
                        write_next(go_on ? (int64_t)r1 + prefix_rank<!SWEEP>(m_push) : (int64_t)r1 + 2 * r + 1, Q->gstage, Q->gstage_cap, LG::STAGE_STRIDE, (int32_t)(cn + 1), 0, -1, -1, fl, 0.0,
                                   o.child_l0, o.oplC, 0.0, 0.0);
                    }
                    kid_here = go_on;
                } else {
                    atomicAdd(&Q->ctr->overflow, 1ull);
                }
            }
        }
        const bool take_kept = valid && alive && !survive && !kid_here && pend_node >= 0;  // this lane's beamlet ends here: it takes up the child it kept
        if (go_on) go_on = __any((survive || kid_here || take_kept) ? 1 : 0) != 0;
        if (go_on) {
            if (valid) {
                if (alive && survive) {
                    int32_t fl, ho, hs;
                    next_header(fl, ho, hs);
                    write_tail(Nq, j, node, k + 1, ho, hs, fl, o.lenA, o.lenB, o.oplC, o.oplW, o.oplD);
                } else if (take_kept) {
                    const int64_t gc = Q->gstage_cap, nc = Nq->cap;
                    BMO_NOUNROLL
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 7; ++c) Nq->d[(LG::RAY_STRIDE * r + c) * nc + j] = Q->gkeep[(int64_t)(LG::STAGE_STRIDE * r + c) * gc + j];
                    write_tail(Nq, j, pend_node, 0, -1, -1, (int32_t)Q->gkeep[LG::KEEP_FLAGS * gc + j], 0.0, Q->gkeep[LG::KEEP_L0 * gc + j], Q->gkeep[LG::KEEP_OPLC * gc + j], 0.0, 0.0);
                    pend_node = -1;
                } else if (!kid_here) {
                    Nq->i[I_NODE * Nq->cap + j] = -1;  // no record of this beamlet at this level
                    alive = false;
                }
            }
            b += 1;
            continue;
        }
        // ---- last fused bounce of this wave
        if constexpr (SWEEP) {  // (a wave's slots are not consecutive: the level is noted per slot, Chunk::wl_shift = 0)
            if (Q->wave_last && valid) Q->wave_last[j] = (uint8_t)b;
        } else if (Q->wave_last && lane_id() == 0) {
            Q->wave_last[gwave] = (uint8_t)b;
        }
        const SlotAlloc al = block_alloc<false, SWEEP>(survive, pend_node >= 0, calls, Q, scratch, b);
        if (survive) {
            const int64_t slot = (int64_t)al.surv_base + prefix_rank<!SWEEP>(al.m_surv);
            int32_t fl, ho, hs;
            next_header(fl, ho, hs);
            write_next(slot, Nq->d, Nq->cap, LG::RAY_STRIDE, node, k + 1, ho, hs, fl, o.lenA, o.lenB, o.oplC, o.oplW, o.oplD);
        }
        if (pend_node >= 0) {  // the reflected children their lanes did not get to
            const int64_t gc = Q->gstage_cap;
            write_next((int64_t)al.child_base + prefix_rank<!SWEEP>(al.m_split), Q->gkeep, gc, LG::STAGE_STRIDE, pend_node, 0, -1, -1, (int32_t)Q->gkeep[LG::KEEP_FLAGS * gc + j], 0.0, Q->gkeep[LG::KEEP_L0 * gc + j],
                       Q->gkeep[LG::KEEP_OPLC * gc + j], 0.0, 0.0);
        }
#if !defined(BMO_NO_TILE_COST)
        if (Q->tile_cost && step_tid<SWEEP>() == 0) Q->tile_cost[tile] = (uint32_t)wall_clock64() - Q->tile_cost[tile];  // (guarded like the start stamp and like step_kernel's)
#endif
        return;
    }
}

// ------------------------------------------------------------------ host side
// The helper kernels sit in the files below, next to the host functions that launch them.
#include "bmo_pool.inc.hpp"

}  // namespace

// ------------------------------------------------------------------ the handles of include/bmo.h
// A scene: the image bmo_scene_blob.hpp built, and its lazily made per-device copies.
struct bmo_scene : SceneImage {
    std::vector<std::pair<int, std::unique_ptr<DevBuf>>> dev;  // per-device copy of the blob
    std::mutex dev_mu;  // the handle is shared between host threads (include/bmo.h "Threading"): the lazy per-device upload is the one mutation
    const char* device_blob(int device, int& rc) {
        std::lock_guard<std::mutex> lk(dev_mu);
        for (auto& d : dev)
            if (d.first == device) return static_cast<const char*>(d.second->p);
        auto b = std::make_unique<DevBuf>();
        rc = b->alloc(blob.size());
        if (rc) return nullptr;
        if (hipMemcpy(b->p, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(BMO_ERR_NO_DEVICE, "hipMemcpy(scene)");
            return nullptr;
        }
        const char* p = static_cast<const char*>(b->p);
        dev.emplace_back(device, std::move(b));
        return p;
    }
};

struct bmo_device_batch {
    int device = 0;
    int kind = 0;
    int64_t n = 0;
    int n_planes = 0;
    DevBuf planes, li;
    DevBuf perm;    // slot -> root ray, roots binned by coherence key (empty: bundle order is kept; root_key_kernel)
    DevBuf binned;  // the planes in slot order (only with perm)
    // feedback for the next solve of this batch (StepParams::tile_order): time of every tile of the first launch, the tiles sorted by it
    DevBuf tile_cost, tile_order, lpt_ids, lpt_keys, lpt_tmp;
    int64_t tile_n = 0;
    bool cost_valid = false;
};

struct bmo_trace_result {
    int device = 0, kind = 0, n_detectors = 0, n_objects = 0;
    int64_t n_roots = 0, n_nodes = 0, n_records = 0;
    unsigned long long calls = 0;
    int n_steps = 0;
    double kernel_ms = 0, total_ms = 0;
    int nd = 0;  // double planes per record (device layout)
    int abi_planes = 0;
    // device state
    std::vector<std::unique_ptr<DevBuf>> arena;  // chunk storage
    int64_t view_records = 0;
    bool has_log = true;                         // false: solved with record_segments = 0, only beams and detector hits were kept
    std::vector<Chunk> chunks;
    std::vector<std::unique_ptr<DevBuf>> wave_last;  // Chunk::wl of the fused launches
    DevBuf n_root, n_parent, n_nseg, n_status, n_li, n_hitdet, n_key, n_lambda, n_hit, n_aux, order, det_data, det_node;
    DevBuf n_old;  // retrace runs only (NodeArrays::old)
    DevBuf pre_start, pre_segs, pre_opl;  // earlier segments of continued root beamlets (bmo_result_set_gauss_prefix), empty otherwise
    int64_t pre_roots = 0, pre_total = 0;
    // tables a later bmo_retrace of THIS solution needs, built on first use (OldSolution)
    std::mutex rt_mu;
    bool rt_built = false;
    DevBuf rt_rec_start, rt_rec_obj, rt_first_child, rt_rec_loc, rt_chunks;
    // time of every tile of this solve's first launch (StepParams::tile_cost), copied from the batch: a retrace of this solution with a
    // freshly uploaded batch (bmo_retrace: the wrappers upload the root heads on every call) orders its tiles by it
    DevBuf tile_cost;
    int64_t tile_n = 0;
    std::vector<int64_t> det_count, det_offset;
    std::vector<int> det_kind;  // object kind recorded into every detector slot (BMO_OBJ_*; -1: none, -2: objects of different kinds)
    // bmo_trace_sweep: configurations of the sweep and the configuration of every root beam (device); 0 / empty for other solves
    int32_t n_configs = 0;
    std::vector<int32_t> root_cfg;
    DevBuf d_root_cfg;
    // host views (filled by bmo_result_view / bmo_result_view_select), all page-locked; each part is materialised on first request
    bool nodes_viewed = false, hits_viewed = false;
    int rec_mode = 0;  // records on the host: 0 none, 1 last segment of every beam, 2 the whole log
    HostBuf h_root, h_parent, h_first_child, h_first_rec, h_last_rec, h_nseg, h_status, h_aux;
    HostBuf h_rec, h_rec_obj, h_rec_shape, h_det, h_det_node;
    DevBuf c_rank, c_first_rec;  // canonical rank of every node id / first record of every canonical node (device, kept for record views)
};

namespace {
#include "bmo_upload.inc.hpp"
#include "bmo_trace_host.inc.hpp"
}  // namespace

// =================================================================== C ABI
extern "C" {

int bmo_version(void) { return BMO_ABI_VERSION; }
#if !defined(BMO_SOURCE_HASH)
#define BMO_SOURCE_HASH ""
#endif
#if !defined(BMO_FLAGS_HASH)
#define BMO_FLAGS_HASH ""
#endif
// (the markers in front let the build script read the hashes out of the file without loading the library; the second one is the hash of
//  the compiler flags, so that a change of flags rebuilds the library too)
const char* bmo_source_hash(void) {
    static const char tagged[] = "BMO_SOURCE_HASH=" BMO_SOURCE_HASH "\0BMO_FLAGS_HASH=" BMO_FLAGS_HASH;
    return tagged + 16;
}
const char* bmo_build_flags_hash(void) {
    static const char tagged[] = "BMO_BUILT_WITH=" BMO_FLAGS_HASH;
    return tagged + 15;
}
const char* bmo_last_error(void) { return g_err.c_str(); }

int bmo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bmo_scene_create(const bmo_scene_desc* d, bmo_scene** out) {
    if (!d || !out) return fail(BMO_ERR_INVALID, "null argument");
    auto sc = std::make_unique<bmo_scene>();
    std::string err;
    if (const int rc = build_scene_image(d, *sc, err)) return fail(rc, err);
    *out = sc.release();
    return BMO_OK;
}

int bmo_scene_create_sweep(const bmo_scene_desc* descs, int32_t n_configs, bmo_scene** out) {
    if (!descs || !out || n_configs < 1) return fail(BMO_ERR_INVALID, "bmo_scene_create_sweep: null argument or n_configs < 1");
    auto sc = std::make_unique<bmo_scene>();
    std::string err;
    if (const int rc = merge_sweep_images(descs, n_configs, *sc, err)) return fail(rc, err);
    *out = sc.release();
    return BMO_OK;
}

int bmo_scene_mesh_bvh(const bmo_scene* scene, int32_t shape, int32_t* n_nodes, int32_t* depth, int32_t* max_leaf) {
    if (!scene) return fail(BMO_ERR_INVALID, "null argument");
    if (shape < 0 || shape >= scene->hdr.n_shapes) return fail(BMO_ERR_INVALID, "shape id out of bounds");
    const BvhStats& st = scene->bvh[(size_t)shape];
    if (n_nodes) *n_nodes = st.n_nodes;
    if (depth) *depth = st.depth;
    if (max_leaf) *max_leaf = st.max_leaf;
    return BMO_OK;
}

int bmo_mesh_nearest_host(const bmo_scene* scene, int32_t shape, int64_t n, const double* pos, const double* dir, double* t, int32_t* fid) {
    if (!scene || n < 0 || (n > 0 && (!pos || !dir || !t || !fid))) return fail(BMO_ERR_INVALID, "null argument");
    if (shape < 0 || shape >= scene->hdr.n_shapes) return fail(BMO_ERR_INVALID, "shape id out of bounds");
    const SceneView S = view_of(scene->blob.data(), &scene->hdr);
    const bmo_shape& sh = S.shapes[shape];
    if (sh.kind != BMO_SHAPE_MESH) return fail(BMO_ERR_INVALID, "not a mesh shape");
    for (int64_t i = 0; i < n; ++i) {
        const d3 p{pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, d{dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]};
        int32_t f = -1;
        t[i] = (sh.flags & BMO_SHAPE_FLAG_BVH) ? mesh_nearest_bvh(S, sh.child_begin, sh.tri_begin, sh.tri_count, p, d, kinf(), f)
                                               : mesh_nearest(S, sh.tri_begin, sh.tri_count, p, d, f);
        fid[i] = f;
    }
    return BMO_OK;
}

int bmo_scene_destroy(bmo_scene* s) {
    delete s;
    return BMO_OK;
}

int bmo_pool_release(void) {
    pool_release_all();
    return BMO_OK;
}

int bmo_batch_upload(bmo_scene* scene, const bmo_ray_batch* in, int32_t device, bmo_device_batch** out) {
    if (scene && scene->n_configs > 1) return fail(BMO_ERR_INVALID, "a sweep scene of several configurations is traced with bmo_trace_sweep");
    return batch_upload(scene, in, device, out, true);
}

int bmo_batch_free(bmo_device_batch* b) {
    if (b) (void)hipSetDevice(b->device);
    delete b;
    return BMO_OK;
}

static int trace_or_retrace(bmo_scene* scene, bmo_device_batch* batch, const bmo_trace_opts* opts, bmo_trace_result* prev, bmo_trace_result** out) {
    if (!scene || !batch || !opts || !out) return fail(BMO_ERR_INVALID, "null argument");
    if (scene->n_configs > 1) return fail(BMO_ERR_INVALID, "a sweep scene of several configurations is traced with bmo_trace_sweep");
    if (prev && prev->n_configs > 0) return fail(BMO_ERR_UNSUPPORTED, "a sweep result cannot be retraced (sweeps are fresh solves of every configuration)");
    if (prev && prev->n_objects != scene->hdr.n_objects)
        return fail(BMO_ERR_INVALID, "retrace: the scene does not have the object numbering the previous solution was solved with");
    auto R = std::make_unique<bmo_trace_result>();
    R->n_objects = scene->hdr.n_objects;
    if (int rc = trace_by_kind(scene, batch, opts, R.get(), prev)) return rc;
    *out = R.release();
    return BMO_OK;
}

int bmo_trace_device(bmo_scene* scene, bmo_device_batch* batch, const bmo_trace_opts* opts, bmo_trace_result** out) {
    return trace_or_retrace(scene, batch, opts, nullptr, out);
}

int bmo_retrace_device(bmo_scene* scene, bmo_device_batch* batch, bmo_trace_result* prev, const bmo_trace_opts* opts, bmo_trace_result** out) {
    if (!prev) return fail(BMO_ERR_INVALID, "retrace: no previous solution");
    return trace_or_retrace(scene, batch, opts, prev, out);
}

int bmo_retrace(bmo_scene* scene, const bmo_ray_batch* in, bmo_trace_result* prev, const bmo_trace_opts* opts, bmo_trace_result** out) {
    if (!scene || !in || !opts || !out || !prev) return fail(BMO_ERR_INVALID, "null argument");
    if (prev->n_configs > 0) return fail(BMO_ERR_UNSUPPORTED, "a sweep result cannot be retraced (sweeps are fresh solves of every configuration)");
    bmo_device_batch* b = nullptr;
    int rc = bmo_batch_upload(scene, in, prev->device, &b);  // the stored solution pins the device
    if (rc) return rc;
    rc = bmo_retrace_device(scene, b, prev, opts, out);
    bmo_batch_free(b);
    return rc;
}

int bmo_trace(bmo_scene* scene, const bmo_ray_batch* in, const bmo_trace_opts* opts, bmo_trace_result** out) {
    if (!opts) return fail(BMO_ERR_INVALID, "null opts");
    bmo_device_batch* b = nullptr;
    int rc = bmo_batch_upload(scene, in, opts->device, &b);
    if (rc) return rc;
    rc = bmo_trace_device(scene, b, opts, out);
    bmo_batch_free(b);
    return rc;
}

int bmo_trace_sweep(bmo_scene* sweep, const bmo_ray_batch* in, const int32_t* root_config, const bmo_trace_opts* opts, bmo_trace_result** out) {
    if (!sweep || !in || !opts || !out) return fail(BMO_ERR_INVALID, "null argument");
    if (sweep->n_configs < 1) return fail(BMO_ERR_INVALID, "bmo_trace_sweep: the scene was not made by bmo_scene_create_sweep");
    if (in->n < 0 || (in->n > 0 && !root_config)) return fail(BMO_ERR_INVALID, "bmo_trace_sweep: root_config missing");
    for (int64_t i = 0; i < in->n; ++i) {
        if (root_config[i] < 0 || root_config[i] >= sweep->n_configs)
            return fail(BMO_ERR_INVALID, "bmo_trace_sweep: root_config[" + std::to_string(i) + "] = " + std::to_string(root_config[i]) + " is not in [0, " +
                                             std::to_string(sweep->n_configs) + ")");
        if (i > 0 && root_config[i] < root_config[i - 1])
            return fail(BMO_ERR_INVALID, "bmo_trace_sweep: root_config decreases at root " + std::to_string(i) + " (the roots of a configuration are consecutive)");
    }
    bmo_device_batch* b = nullptr;
    int rc = batch_upload(sweep, in, opts->device, &b, false);
    if (rc) return rc;
    std::unique_ptr<bmo_device_batch, int (*)(bmo_device_batch*)> hold_b(b, bmo_batch_free);
    auto R = std::make_unique<bmo_trace_result>();
    R->n_objects = sweep->hdr.n_objects;
    R->n_configs = sweep->n_configs;
    R->root_cfg.assign(root_config, root_config + in->n);
    if ((rc = R->d_root_cfg.alloc((size_t)std::max<int64_t>(in->n, 1) * 4))) return rc;
    if (in->n) HIP_TRY(hipMemcpy(R->d_root_cfg.p, root_config, (size_t)in->n * 4, hipMemcpyHostToDevice));
    if ((rc = trace_by_kind(sweep, b, opts, R.get(), nullptr))) return rc;
    *out = R.release();
    return BMO_OK;
}

int bmo_result_free(bmo_trace_result* r) {
    if (r) (void)hipSetDevice(r->device);
    delete r;
    return BMO_OK;
}

}  // extern "C"

#include "bmo_result_view.inc.hpp"
#include "bmo_selftest.inc.hpp"
#include "bmo_readout.inc.hpp"
