// MI355X (gfx950) bitHTM timestep engine: HIP kernels + the C ABI of include/bithtm_hip.h.
//
// One handle = all device state of one SpatialPooler + TemporalMemory pair.  A timestep is a
// fixed sequence of kernel launches on one stream with NO host synchronisation: every
// data-dependent size (segments, matching segments, winners, work items) lives in a device
// counter block and kernels grid-stride over those counters.
//
// Semantics follow the reference lines cited next to each kernel (paths relative to the
// reference checkout) under the deterministic policies of DESIGN.md.  Compile with
// -ffp-contract=off: several kernels must round exactly like the NumPy expressions they replace.
//
// Internal cell encoding: enc = column * KP + cell, KP = 32 cell slots per column (one 32-bit word per column in the dense
// bitmaps) or 64 for cell_dim above 32 (two words);
// the ABI converts to / from the reference's flat id column * cell_dim + cell.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/bithtm_hip.h"
#include "htm_fexp.h"
#include "htm_rng.h"

#include "htm_dev.h"
#include "htm_sp_kernels.h"
#include "htm_tm_kernels.h"
#include "htm_pipeline.h"
#include "htm_record.h"
#include "htm_reset.h"
#include "htm_decode.h"
#include "htm_stack.h"
#include "htm_pool.h"
#include "htm_forecast.h"
#include "htm_noise.h"
#include "htm_group.h"
#include "htm_tm_feed.h"
#include "htm_sp_run.h"
#include "htm_fork.h"
#include "htm_scalar.h"
#include "htm_live.h"
#include "htm_fields.h"
#include "htm_coord.h"
#include "htm_likelihood.h"
#include "htm_classifier.h"
#include "htm_knn.h"
#include "htm_knn_bank.h"
#include "htm_handover.h"
#include "htm_handover_last.h"
#include "htm_group_stack.h"

// ------------------------------------------------------------------------------------------
// host side

struct ncclUniqueIdBytes { char internal[128]; };      // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES), passed by value

static thread_local std::string g_create_error;
static int (*g_rccl_destroy)(void *) = nullptr;        // ncclCommDestroy once RCCL is loaded

// The environment's knobs (tuning and test knobs), read when a handle is created (read_knobs; an inference view takes its
// parent's: htm_create_view).  The knobs of launch sizes read 0 when they are not given (a given one is at least 1), and
// BITHTM_SEL_LAUNCH_DIGITS -1: size_launches derives those.
struct Knobs {
    int graph_steps, eager_below;         // BITHTM_GRAPH_STEPS, BITHTM_EAGER_BELOW
    bool trace;                           // BITHTM_TRACE given (and BITHTM_TRACE_UNTIL)
    uint32_t trace_until;
    int lean, lean2_classify, lean2_order, step_split, fuse_tm, shard_window, step_window, tail_rows, scan_large, scan_large_above, scan_dyn;
    int defer_tail, shared_scan, shared_members;
    int handover_cap;                     // BITHTM_HANDOVER_LDS_CAP (test knob)
    int lean_overlap, lean_learn, lean_learn_large, lean_scan, lean_scan_large, scan_blocks, sel_launch_digits;
    int cand_d, cand_pairwise, cls_rows_max, win_offset, cand_zoom, cand_speculate, cand_take_all, poll_delay, cand_others;   // (Dev's)
};

// Launch sizes of a handle, derived once from its shape, its knobs and the device (size_launches)
struct Sizes {
    int G;                                // lanes per SP row
    int sp_blocks, sel_blocks, c256_blocks, s1024_blocks, scan_blocks, zero_blocks, cus;
    int lean_learn_blocks, lean_learn_blocks_large, lean_scan_blocks, lean_scan_blocks_large, lean_overlap_blocks, lean2_classify_blocks;
    int lean2_overlap_blocks;             // blocks of k_act_mid_rows' overlap role: 256 columns each where it reads the byte planes (role_overlap_planes)
    int lean_resident_large;              // blocks of the large-pool k_learn_scan_emit that are resident at once
    bool emit_fits, emit_fits_open;       // the emit grid is resident at once in k_sp_emit / in k_open_emit, as far as this handle's own grids go
    bool emit_fits_lean;                  // ... and in k_learn_scan_emit
    int sel_passes_fused, sel_passes_full; // launched select digits with / without the in-kernel finish
};

// The modes of one batched call -- its steps are recorded, reset by the bank's bits, decoded, fed back -- as its setup returns them
// (begin_run_modes, group_begin_modes).  Whatever enqueues or captures a step takes them by value; a host-fed step has none.
struct RunModes {
    bool recording, resetting, decoding, feeding;
    bool capturing = false;               // htm_set_run_active_cells: a recorded htm_run whose steps leave their active-cell words
    bool operator<(const RunModes &o) const {
        return std::tie(recording, resetting, decoding, feeding, capturing) < std::tie(o.recording, o.resetting, o.decoding, o.feeding, o.capturing);
    }
};

// What the launches of a captured graph depend on besides the handle's fixed sizes.  htm_run: the step's parity, the call's
// modes, its StepPlan and schedule, the scan's form, the span of steps, the bank
struct RunGraphKey {
    int p; RunModes modes; int learning; bool sp_done, next_sp, next_front, lean; int spec; bool large, emit_fused, wmode;
    int span; const void *bank; int n_inputs;
    auto tie() const { return std::tie(p, modes, learning, sp_done, next_sp, next_front, lean, spec, large, emit_fused, wmode, span, bank, n_inputs); }
    bool operator<(const RunGraphKey &o) const { return tie() < o.tie(); }
};

// ... htm_shard_run / htm_shard_group_run: per rank the scan blocks known to have segments, the scan's form and the exchange mode;
// rank 0's bank
struct ShardGraphKey {
    int p, learning; bool front_done, front_next; int span, ranks, n_inputs; std::vector<std::tuple<int, bool, bool>> per_rank; const void *bank;
    auto tie() const { return std::tie(p, learning, front_done, front_next, span, ranks, n_inputs, per_rank, bank); }
    bool operator<(const ShardGraphKey &o) const { return tie() < o.tie(); }
};

// ... htm_tm_run: the step's parity, the call's modes, the scan's form, the span of steps, the bank of lists and its shape
struct TmRunGraphKey {
    int p; RunModes modes; int learning, spec; bool large; int span; const void *lists; int n_rows, n;
    auto tie() const { return std::tie(p, modes, learning, spec, large, span, lists, n_rows, n); }
    bool operator<(const TmRunGraphKey &o) const { return tie() < o.tie(); }
};

// ... htm_sp_run: the step's parity, the learning flag, whether the steps are recorded, the form of the select (launched count or
// in-kernel finish; digits or window), the span of steps, the bank
struct SpRunGraphKey {
    int p, learning; bool recording, emit_fused; int wmode, span; const void *bank; int n_inputs;
    auto tie() const { return std::tie(p, learning, recording, emit_fused, wmode, span, bank, n_inputs); }
    bool operator<(const SpRunGraphKey &o) const { return tie() < o.tie(); }
};

struct htm_handle {
    htm_config cfg;
    Dev d;
    Knobs knob;
    Sizes sz;
    int device;
    hipStream_t stream;
    bool own_stream;
    long long step_host;
    std::string err;
    std::vector<void *> allocs;
    int *d_cols_stage;                    // stand-alone TM: active columns
    int rank, world;                      // column sharding
    const uint32_t *shard_bank;           // input of the step between htm_shard_begin and _finish
    int shard_n_inputs = 1;
    bool shard_open;
    bool shard_graph_ok;                  // htm_shard_comm_init's preflight: this communicator's all-gather replays correctly from a captured hipGraph
    int shard_front_wmode;                // htm_shard_run: the histogram form of the overlap computed ahead for the coming step
    std::map<ShardGraphKey, hipGraphExec_t> shard_graphs;     // (on rank 0's handle for a group in one process)
    void *rccl_comm;                      // ncclComm_t of htm_shard_comm_init (the exchange of htm_shard_step)
    unsigned char *shard_send, *shard_recv;   // ... and its device buffers
    bool emit_fused, emit_fused_open;     // the emit grid is resident at once in k_sp_emit / in k_open_emit (refreshed per call)
    bool tail_pending;                    // htm_step holds back the learning role and the scan of the step of parity tail_p
    int tail_p;
    bool window_known;                    // a select has run on this handle since it was created / imported into: Counters::sel_win is meaningful
    int seg_hint;                         // a lower bound of the segment count (see scan_spec_blocks)
    int *seg_pinned;                      // pinned word the end of each htm_run copies the count into
    const uint32_t *ahead_bank;           // htm_run ended with HTM_RUN_CONTINUE on this bank: the SP has done the next step
    int ahead_n_inputs, ahead_learning;   //   and the front of the one after it
    bool ahead_lean;                      //   ... in the three-launch schedule (else the four-launch one)
    int phase_active;                     // htm_sp_phase: length of the current winner list
    bool phase_wide;                      // ... the keys of the current step were made from values the HOST supplied (BOOST, SELECT with
                                          // data): nothing bounds their significant bits, the select resolves all 64 key bits
    bool import_keep;                     // htm_import_begin(HTM_IMPORT_PREV_STATE): the commit leaves the store, the step index and the sticky flags alone
    bool phase_open;                      // ... phases of the current (not yet closed) timestep have run: the Spatial Pooler
                                          // fields htm_read returns are that step's
    RecDev *d_rec;                        // recorded runs (htm_run_recorded): the device descriptor every record launch reads (filled by each such call)
    // sequence resets of htm_run (htm_set_run_resets): the caller's device bits and bank size, and the device descriptor the reset
    // launches read (filled by each call that has bits)
    const uint32_t *reset_bits;
    int reset_n;
    ResetDev *d_reset;
    // predicted-input decoding (htm_set_run_predicted_input): the caller's device rows, the device descriptor the decoding
    // launches read (filled by each call that decodes), and the output row of htm_predicted_input
    int32_t *pin_out;
    PinDev *d_pin;
    int32_t *d_pin_buf;
    int32_t *d_value_out;                           // htm_predicted_value: the (bucket, score) pairs of its decode launch
    // pattern capture (htm_set_run_active_cells): the caller's device rows and the device descriptor the capture launches read
    // (filled when the rows are set)
    void *cap_out = nullptr;
    ClsCapDev *d_cap = nullptr;
    // run feedback (htm_set_run_feedback): the bank whose runs write their next row and its size, the device descriptor the
    // feedback launches read (filled when the feedback is set), and the scratch votes row (zero between uses: htm_forecast.h)
    uint32_t *feed_bank;
    int feed_n;
    FeedDev *d_feed;
    int32_t *d_feed_votes;
    std::map<RunGraphKey, hipGraphExec_t> graphs;
    std::map<TmRunGraphKey, hipGraphExec_t> tm_graphs;        // htm_tm_run
    std::map<SpRunGraphKey, hipGraphExec_t> sp_graphs;        // htm_sp_run
    SpRecDev *d_sp_rec;                   // ... its recorded calls: the device descriptor the tail launches read (filled by each such call)
    // state import staging (htm_write of the MATCH_* / SEG_POTENTIAL fields, applied at commit)
    std::vector<int> imp_pot, imp_match_seg;
    // ... on a column-sharded handle also the per-segment arrays (written for ALL segment ids; the commit keeps the rows of
    // the segments this rank's cells own)
    std::vector<int> imp_seg_cell, imp_seg_nsyn, imp_presyn;
    std::vector<float> imp_perm;
    std::vector<uint32_t> imp_match_info;
    std::vector<float> imp_match_jit;
    // profiling
    bool profile;
    hipEvent_t prof_last;                  // event closing the previous kernel of the profiled chain
    std::vector<hipEvent_t> prof_all;      // every event created (destroyed in htm_profile_read)
    std::vector<std::string> prof_names;
    std::vector<std::vector<std::pair<hipEvent_t, hipEvent_t>>> prof_events;
    std::vector<double> prof_ms;
    std::vector<long long> prof_n;
    // inference views (htm_create_view): the weights' allocations while the handle has no view (then they move to `shared`),
    // the reference-counted weights a parent and its views share, whether this handle is a view, and the weights' generation
    // (HtmShared::wgen) the view's per-cell maxima were last made against
    std::vector<void *> weight_allocs;
    struct HtmShared *shared;
    bool is_view;
    long long seen_wgen;
    uint32_t dense_step;                  // (the host word a view's counter block takes cm_dense_step from)
    int64_t own_bytes;                    // device bytes this handle allocated itself (htm_device_bytes)
    unsigned long long *d_planes_bad;     // htm_sp_planes_check's count (allocated by its first call)
};

// The weights of a parent and its inference views (htm_create_view): freed, with the parent's own stream if it created one, when
// the last of them is destroyed.  parent: null once the parent is destroyed (its weights then no longer change).  wgen: bumped by
// every parent call that may change the weights (weights_touched).
struct HtmShared {
    std::vector<void *> allocs;
    hipStream_t stream;
    bool own_stream;
    htm_handle *parent;
    int refs;
    long long wgen;
};
static std::mutex g_shared_mutex;

// Live handles, per process.  The in-kernel select finish (k_sp_emit / k_open_emit) makes the blocks of one grid
// wait for each other, which is only safe while nothing else can hold the CU slots that grid needs: kernels of
// one stream run one after the other, kernels of another handle's stream do not.  A handle therefore uses the
// in-kernel finish only while every other live handle on its device enqueues on the same stream; otherwise it
// launches all select digits and the separate count kernel (slower, no waiting between blocks, same result).
static std::mutex g_registry_mutex;
static std::vector<htm_handle *> g_registry;

static void refresh_exchange_mode(htm_handle *h) {
    bool solo = true;
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        for (const htm_handle *o : g_registry)
            if (o != h && o->device == h->device && o->stream != h->stream) solo = false;
    }
    h->emit_fused = h->sz.emit_fits && solo;
    h->emit_fused_open = h->sz.emit_fits_open && solo;
    h->d.sel_passes = h->emit_fused ? h->sz.sel_passes_fused : h->sz.sel_passes_full;
}

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return HTM_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

// the Spatial Pooler is ahead of the Temporal Memory across a call boundary (htm_run with HTM_RUN_CONTINUE): only the
// continuing htm_run may come next
static bool sp_is_ahead(const htm_handle *h) { return h->ahead_bank != nullptr; }
#define REJECT_WHEN_AHEAD(h)                                                                                      \
    do {                                                                                                          \
        if (sp_is_ahead(h)) {                                                                                     \
            (h)->err = "the Spatial Pooler is ahead (htm_run ended with HTM_RUN_CONTINUE): continue with htm_run on the same bank"; \
            return HTM_ERR_STATE;                                                                                 \
        }                                                                                                         \
    } while (0)

// the status of the launches just enqueued
static int launch_status(std::string &err) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HTM_OK;
    err = std::string("kernel launch: ") + hipGetErrorString(e);
    return HTM_ERR_HIP;
}

// the segment count the end of the last run left in the pinned word (read without a wait: a lower bound) ...
static void refresh_seg_hint(htm_handle *h) {
    if (h->seg_pinned) h->seg_hint = std::max(h->seg_hint, (int)*(volatile int *)h->seg_pinned);
}

// ... and the copy that leaves it there, queued at the end of a run: `count` is the counter of the rows the scan covers
// (&Counters::S, or a shard's &Counters::L)
static hipError_t hand_back_segments(htm_handle *h, const int32_t *count, hipStream_t stream) {
    return h->seg_pinned ? hipMemcpyAsync(h->seg_pinned, count, sizeof(int), hipMemcpyDeviceToHost, stream) : hipSuccess;
}

// The graph `key` names in `graphs`: found, or what `enqueue` launches captured on `stream` (enqueue returns 0, or an error
// status with err set), instantiated and kept.  nullptr: the capture or the instantiation failed (err says which).  The
// captured hipGraph_t is destroyed either way.
template <typename Key, typename Enqueue>
static hipGraphExec_t cached_graph(std::map<Key, hipGraphExec_t> &graphs, const Key &key, hipStream_t stream, std::string &err, Enqueue enqueue) {
    auto it = graphs.find(key);
    if (it != graphs.end()) return it->second;
    hipError_t e = hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { err = std::string("hipStreamBeginCapture: ") + hipGetErrorString(e); return nullptr; }
    const int rc = enqueue();
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    e = hipStreamEndCapture(stream, &graph);
    if (rc) {
    } else if (e != hipSuccess || !graph) {
        err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e);
    } else if ((e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0)) != hipSuccess) {
        err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e);
        exec = nullptr;
    }
    if (graph) hipGraphDestroy(graph);
    if (exec) graphs.emplace(key, exec);
    return exec;
}

template <typename T>
static int dalloc(htm_handle *h, T **p, size_t count) {
    void *q = nullptr;
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) {
        h->err = "hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
        return HTM_ERR_HIP;
    }
    e = hipMemsetAsync(q, 0, bytes, h->stream);
    if (e != hipSuccess) { h->err = std::string("hipMemsetAsync: ") + hipGetErrorString(e); return HTM_ERR_HIP; }
    h->allocs.push_back(q);
    h->own_bytes += (int64_t)bytes;
    *p = (T *)q;
    return 0;
}

// ... of the weights (what an inference view aliases instead of allocating)
template <typename T>
static int dalloc_weights(htm_handle *h, T **p, size_t count) {
    const int rc = dalloc(h, p, count);
    if (!rc) { h->weight_allocs.push_back(h->allocs.back()); h->allocs.pop_back(); }
    return rc;
}

static int prof_slot(htm_handle *h, const char *name) {
    for (size_t i = 0; i < h->prof_names.size(); ++i)
        if (h->prof_names[i] == name) return (int)i;
    h->prof_names.push_back(name);
    h->prof_events.emplace_back();
    h->prof_ms.push_back(0.0);
    h->prof_n.push_back(0);
    return (int)h->prof_names.size() - 1;
}

// Profiling: hipExtLaunchKernelGGL stamps a start and a stop event with the kernel's own begin /
// end timestamps on the device -- the quantity rocprofv3's kernel trace reports -- so the two can
// be compared directly (an event recorded between launches would add its marker and the dependent
// launch gap to every kernel).
#define LAUNCH_ON(h, strm, shmem, name, kernel, grid, block, ...)                                 \
    do {                                                                                         \
        if ((h)->profile) {                                                                      \
            hipEvent_t e0_ = nullptr, e1_ = nullptr;                                             \
            hipEventCreate(&e0_);                                                                \
            hipEventCreate(&e1_);                                                                \
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, strm, e0_, e1_, 0, __VA_ARGS__); \
            (h)->prof_events[prof_slot(h, name)].push_back({e0_, e1_});                          \
        } else {                                                                                 \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, strm, __VA_ARGS__);       \
        }                                                                                        \
    } while (0)
#define LAUNCH(h, name, kernel, grid, block, ...) LAUNCH_ON(h, (h)->stream, 0, name, kernel, grid, block, __VA_ARGS__)

static size_t learn_lds(int epl, int bs = RB) { return (size_t)(bs / 64) * CAND_CAP * 8 + (size_t)(bs / 64) * epl * 64 * 4 + (size_t)WIN_LDS * 4; }
static int learn_epl(const Dev &d) { const int e = d.E / 64; return e <= 1 ? 1 : e == 2 ? 2 : e <= 4 ? 4 : 8; }
// (... and, behind the bitmap, the queues in which the waves of the streaming form set rows aside: 32 entries of 12 bytes per wave)
static size_t scan_lds(const Dev &d, int use_lds) { return 16 + (use_lds ? (size_t)((d.colwords + 3) & ~3) * 4 : 0) + 4 * 32 * 12; }
// ... with the rank of every bitmap word and the active words of the step's active columns behind the bitmap (the
// three-launch schedule's scan looks the cells of active columns up in LDS: role_scan, TAB)
static size_t scan_lds_tab(const Dev &d) {
    return 16 + (size_t)((d.colwords + 3) & ~3) * 4 + (size_t)((d.colwords * 2 + 15) / 16) * 16 + (size_t)((d.k * d.WPC + 8 + 3) / 4) * 16;
}
// ... which needs them to fit (and the ranks 16 bits); otherwise the schedule's scan reads the cell words from memory
static bool lean_tab(const Dev &d) { return scan_lds_tab(d) <= 64 * 1024 && d.k * d.WPC < 65536; }
static size_t lean_scan_lds(const Dev &d) { return lean_tab(d) ? scan_lds_tab(d) : scan_lds(d, 1); }
// the scan's column bitmap fits the LDS
static bool bitmap_fits_lds(const Dev &d) { return scan_lds(d, 1) <= 64 * 1024; }
// activation blocks of a step: one active column per lane group of a 256-thread block (role_activate)
static int act_blocks(const Dev &d) { return (d.k * d.KP + 255) / 256; }
static const int kClassifyBlocks = 384;           // x 256 segments per pass of the learn / punish classification
static const int kLearnBlocks = 256;               // x RB/64 waves: one wave per learning / punished segment

// Each family of kernel instantiations is a table (kt_*), by the learning role's width (learn_epl: 1, 2, 4, 8 -> epl_slot) or by
// the scan's form (scan_slot: large pool with / without the column bitmap in LDS, small pool with / without it).  A table stands
// before the first launch from it: the order in which kernels are first named is the order of their code in the code object.
static int epl_slot(const Dev &d) { const int e = learn_epl(d); return e == 1 ? 0 : e == 2 ? 1 : e == 4 ? 2 : 3; }
static int scan_slot(bool large, bool use_lds) { return (large ? 0 : 2) + (use_lds ? 0 : 1); }
static decltype(&k_tm_learn<1>) const kt_tm_learn[4] = {k_tm_learn<1>, k_tm_learn<2>, k_tm_learn<4>, k_tm_learn<8>};

static void launch_learn(htm_handle *h, int p) {
    LAUNCH_ON(h, h->stream, learn_lds(learn_epl(h->d)), "tm_learn", kt_tm_learn[epl_slot(h->d)], kLearnBlocks, RB, h->d, p);
}

// scan blocks that certainly have segments: the count only grows, and the host sees it now and then
// (htm_get_info, state import, and a copy queued at the end of every htm_run)
// (rounded down to a multiple of 64 blocks: the value is baked into captured graphs)
static int scan_spec_blocks(const htm_handle *h) { return std::min(h->seg_hint / SCAN_SEGS, h->sz.scan_blocks) & ~63; }

// more segments than three rounds of resident blocks: the scan is bandwidth-bound (see k_tm_scan)
static bool scan_pool_is_large(const htm_handle *h) {
    if (h->knob.scan_large >= 0) return h->knob.scan_large != 0;      // (BITHTM_SCAN_LARGE: tuning knob)
    return h->seg_hint > h->knob.scan_large_above;
}

static void launch_scan(htm_handle *h, int p, int use_lds) {
    Dev &d = h->d;
    const int spec = scan_spec_blocks(h);
    if (scan_pool_is_large(h) && use_lds && scan_lds(d, 1) > 16 * 1024) {
        // a big column bitmap (32 KB at 262 144 columns): one copy per 1024-thread block, two blocks per CU
        const int blocks = std::max(1, std::min((d.Lcap + 255) / 256, 2 * h->sz.cus));
        LAUNCH_ON(h, h->stream, scan_lds(d, 1), "tm_scan_wide", (k_tm_scan_wide<true>), blocks, 1024, d, p, 0);
        return;
    }
    static decltype(&k_tm_scan<true, 1>) const kt_tm_scan[4] = {k_tm_scan<true, 1>, k_tm_scan<false, 1>, k_tm_scan<true, 6>, k_tm_scan<false, 6>};
    const bool large = scan_pool_is_large(h);
    LAUNCH_ON(h, h->stream, scan_lds(d, use_lds), large ? "tm_scan_large" : "tm_scan", kt_tm_scan[scan_slot(large, use_lds)], h->sz.scan_blocks, 256, d, p, spec);
}

// the windowed one-pass select (win_bin) outside the three-launch schedule too: the histogram is finished inside the emit
// grid, so only where that grid's blocks may wait for each other (BITHTM_STEP_WINDOW=0: two launched digits, as before)
// (and only once a select has left a window behind: the first step of a handle, or after a state import, takes the digits)
static int step_wmode(const htm_handle *h) { return h->emit_fused && h->knob.step_window && h->world == 1 && h->window_known ? 1 : 0; }

// a host-fed step's packed input as a launch argument (where it fits: d.W <= ARG_INPUT_WORDS)
static PackedInputArg packed_input_arg(const Dev &d, const uint32_t *host_input) {
    PackedInputArg in;
    memset(&in, 0, sizeof(in));
    memcpy(in.w, host_input, (size_t)((d.I + 31) / 32) * 4);
    return in;
}

// the select digits behind the top one, a launch each (d: the handle's descriptor, or a copy with more digits: htm_sp_phase)
static void launch_sel_passes(htm_handle *h, const Dev &d, int p) {
    for (int pass = 1; pass < d.sel_passes; ++pass) LAUNCH(h, "sp_select", k_sel_pass, h->sz.sel_blocks, RB, d, pass, p);
}

// the top-digit histogram of parity p starts clean again: its overlap was computed and no select will consume (and clear) it
static hipError_t clear_front_hist(htm_handle *h, int p) {
    return hipMemsetAsync(h->d.hist0 + (size_t)p * HIST0_PAR, 0, (size_t)HIST0_PAR * 4, h->stream);
}

// Front of SpatialPooler.process for the step with parity sp: overlap + boost + histogram (the windowed one, or the top
// key digit and then the remaining select digits).  host_input: the packed input of a host-fed step (it rides in the
// launch's arguments where it fits); else the bank in device memory.
static void enqueue_sp_front(htm_handle *h, const uint32_t *bank, int n_inputs, int p, int wmode, const uint32_t *host_input = nullptr) {
    Dev &d = h->d;
    if (host_input && d.W <= ARG_INPUT_WORDS) {
        LAUNCH(h, "sp_overlap", k_sp_overlap_arg, h->sz.sp_blocks, RB, d, packed_input_arg(d, host_input), h->sz.G, p, wmode);
    } else {
        LAUNCH(h, "sp_overlap", k_sp_overlap, h->sz.sp_blocks, RB, d, bank, n_inputs, h->sz.G, p, p, 0, wmode);
    }
    if (!wmode) launch_sel_passes(h, d, p);
}

// Rest of SpatialPooler.process: count + emit.  mode = EMIT_ALL: all of it, with the TM's per-column
// activation when the handle has a Temporal Memory.  sp_learn: the permanence update as a launch of
// its own (handles without a Temporal Memory, and the first step of a pipelined run).
static void enqueue_sp_back(htm_handle *h, const uint32_t *bank, int n_inputs, int p, int want_winner, int mode, bool sp_learn, int wmode = 0) {
    Dev &d = h->d;
    const int fused = h->emit_fused;               // all blocks co-resident: count inside emit
    if (!fused) LAUNCH(h, "sp_count", k_sp_count, h->sz.c256_blocks, 256, d, p);
    LAUNCH(h, "sp_emit", k_sp_emit, h->sz.c256_blocks, 256, d, p, want_winner, fused, mode, fused ? wmode : 0, h->sz.c256_blocks);
    h->window_known = true;                         // (every select leaves the next step's window behind)
    // (a forked graph branch for this independent update was measured at +17..29 us per step on
    // this runtime, against 2.3 us for one more kernel in the chain: tools/launch_overhead.hip)
    if (sp_learn) LAUNCH(h, "sp_learn", k_sp_learn, d.k, 256, d, bank, n_inputs, p);
}

// TemporalMemory.process after the per-column activation, one role per launch.  sp_rows: the SP
// permanence update of this step rides along in the middle launch.
// front_wmode >= 0 (column-sharded handles inside htm_shard_run): the overlap of the COMING step on the rank's own
// columns rides in the last launch (wmode = front_wmode: windowed histogram or top digit)
// the learning role and the scan: one launch (the learning waves scan their own rows), unless the pool is large (the
// streaming scan kernels) or somebody is timing the roles one by one (unsharded handles under htm_profile)
static bool tm_tail_fused(const htm_handle *h) {
    return h->knob.fuse_tm && !(h->profile && h->world == 1) && !scan_pool_is_large(h) && bitmap_fits_lds(h->d);
}

// Sizes of a launch that begins with the learning role and the small-pool scan (the plain k_learn_scan_emit, k_learn_scan_tail,
// k_learn_scan_front, kgrp_tail): slot in the kt_* tables, blocks of the two roles, the scan's speculation, and the LDS --
// the larger of the two roles' and of extra_lds, what the role riding behind them needs.  That role's blocks are added where
// it is launched.
struct LearnScan {
    int slot, n_learn, n_scan, spec;
    size_t lds;
    int blocks() const { return n_learn + n_scan; }
};
static LearnScan learn_scan(const htm_handle *h, size_t extra_lds = 0) {
    const Dev &d = h->d;
    return {epl_slot(d), h->sz.lean_learn_blocks, h->sz.lean_scan_blocks, scan_spec_blocks(h),
            std::max(std::max(learn_lds(learn_epl(d), 256), scan_lds(d, 1)), extra_lds)};
}

// k_learn_scan_emit by the form of its scan (lse_kernel): the small-pool scan without its LDS tables (what the fused tail launches) ...
enum { LSE_TAB, LSE_PLAIN, LSE_LARGE };
static decltype(&k_learn_scan_emit<1, 6>) const kt_lse_plain[4] = {k_learn_scan_emit<1, 6, false>, k_learn_scan_emit<2, 6, false>,
                                                                   k_learn_scan_emit<4, 6, false>, k_learn_scan_emit<8, 6, false>};

// the learning role and the scan of the step of parity p, nothing beside them
static void enqueue_tm_tail(htm_handle *h, int p) {
    Dev &d = h->d;
    if (tm_tail_fused(h)) {
        const LearnScan ls = learn_scan(h);
        LAUNCH_ON(h, h->stream, ls.lds, "tm_learn+tm_scan", kt_lse_plain[ls.slot], ls.blocks(), 256, d, p, 0, ls.n_learn, ls.n_scan, ls.spec);
    } else {
        launch_learn(h, p);
        launch_scan(h, p, bitmap_fits_lds(d));
    }
}

// htm_step may hold a step's last launch back (the next call's first launch carries it beside its overlap): everything else
// that touches the handle lets it go first
static void flush_tail(htm_handle *h) {
    if (!h->tail_pending) return;
    h->tail_pending = false;
    hipSetDevice(h->device);
    enqueue_tm_tail(h, h->tail_p);
}

static decltype(&k_learn_scan_tail<1>) const kt_learn_scan_tail[4] = {k_learn_scan_tail<1>, k_learn_scan_tail<2>, k_learn_scan_tail<4>, k_learn_scan_tail<8>};

// defer_tail: the last launch is held back (htm_step: see flush_tail); the permanence rows then ride in the middle launch
static void enqueue_tm(htm_handle *h, int n_active, int learning, int want_winner, int p,
                       const uint32_t *bank, int n_inputs, bool sp_rows, int front_wmode = -1, bool defer_tail = false) {
    Dev &d = h->d;
    const int n_cls = learning ? kClassifyBlocks : 0;
    const bool fuse = tm_tail_fused(h);
    int n_sp_rows = (sp_rows && learning && h->cfg.enable_sp) ? d.k : 0;
    // an unsharded step's permanence rows ride in that launch (the middle launch is left with the Temporal Memory's chain);
    // a shard's stay in the middle launch: the coming step's overlap, which reads them, may ride in the last one
    const int n_tail_rows = (fuse && h->world == 1 && h->knob.tail_rows && !defer_tail) ? n_sp_rows : 0;
    if (n_tail_rows) n_sp_rows = 0;
    const int n_duty = h->world > 1 ? (d.c1 - d.c0 + 255) / 256 : 0;      // (unsharded: the emit role updates the duty cycle)
    LAUNCH(h, "tm_mid", k_mid_rows, 1 + n_cls + n_sp_rows + n_duty + h->sz.zero_blocks, 256, d, p, n_active, want_winner, learning, n_cls, bank, n_inputs, n_sp_rows, 0, n_duty);
    if (defer_tail) { h->tail_pending = true; h->tail_p = p; return; }
    if (fuse && (front_wmode >= 0 || n_tail_rows)) {
        const LearnScan ls = learn_scan(h, (size_t)SEL_BINS * 4);
        const int grid = ls.blocks() + (n_tail_rows ? n_tail_rows : h->sz.lean_overlap_blocks);
        const char *name = n_tail_rows ? "tm_learn+tm_scan+sp_learn" : "tm_learn+tm_scan+shard_overlap";
        LAUNCH_ON(h, h->stream, ls.lds, name, kt_learn_scan_tail[ls.slot], grid, 256, d, p, ls.n_learn, ls.n_scan, ls.spec, bank, n_inputs, h->sz.G, front_wmode, n_tail_rows);
        return;
    }
    enqueue_tm_tail(h, p);
    // (a large pool streams through kernels of its own: the front as a launch behind them)
    if (front_wmode >= 0)
        LAUNCH(h, "shard_overlap", k_shard_overlap, h->sz.sp_blocks, RB, d, bank, n_inputs, h->sz.G, p, front_wmode, 1);
}

// How a step is launched inside htm_run.
//   sp_done   the Spatial Pooler has already done this step (winner list, permanence rows, duty cycle)
//   next_sp   finish the SP's next step beside this step's TM (winner list, rows, duty cycle; its
//             overlap and select digits were computed one step earlier, or by the cold start)
//   next_front  compute overlap + select digits of the step after the next
// The look-ahead includes the SP's persistent updates, so it only ever happens between steps of one
// htm_run call (same bank, same learning flag): the last step of a run has neither, the one before it
// no next_front, and no call returns with SP work outstanding.
struct StepPlan { bool sp_done, next_sp, next_front; };

// the pipelined schedule needs the select finished inside one co-resident emit grid after two
// launched digits
static bool can_pipeline(const htm_handle *h) {
    return h->cfg.enable_sp && h->cfg.enable_tm && h->world == 1 && h->emit_fused_open && h->d.sel_passes == 2;
}

// the three-launch schedule (htm_pipeline.h): the scan's LDS bitmap, one select histogram, the learning role and the
// scan in one launch.  BITHTM_LEAN=0: the four-launch schedule below.
static bool can_lean(const htm_handle *h) {
    return h->knob.lean && can_pipeline(h) && bitmap_fits_lds(h->d) && h->sz.emit_fits_lean;
}

// ... the streaming large-pool scan (which reads the cell words from memory: with the LDS tables it measured 3 % slower -- the
// LDS pipe is one of the things that bound it), and the small-pool scan with its LDS tables (lean_tab)
static decltype(&k_learn_scan_emit<1, 6>) const kt_lse_large[4] = {k_learn_scan_emit<1, 4, false>, k_learn_scan_emit<2, 4, false>,
                                                                   k_learn_scan_emit<4, 4, false>, k_learn_scan_emit<8, 4, false>};
static decltype(&k_learn_scan_emit<1, 6>) const kt_lse_tab[4] = {k_learn_scan_emit<1, 6, true>, k_learn_scan_emit<2, 6, true>,
                                                                 k_learn_scan_emit<4, 6, true>, k_learn_scan_emit<8, 6, true>};
// ... and the forms with the list role at the end of the grid (k_last_handover, htm_handover_last.h): the last launch of a step
// whose first launch is k_first_handover
static decltype(&k_learn_scan_emit<1, 6>) const kt_lsel_large[4] = {k_last_handover<1, 4, false>, k_last_handover<2, 4, false>,
                                                                    k_last_handover<4, 4, false>, k_last_handover<8, 4, false>};
static decltype(&k_learn_scan_emit<1, 6>) const kt_lsel_tab[4] = {k_last_handover<1, 6, true>, k_last_handover<2, 6, true>,
                                                                  k_last_handover<4, 6, true>, k_last_handover<8, 6, true>};
static decltype(&k_learn_scan_emit<1, 6>) const kt_lsel_plain[4] = {k_last_handover<1, 6, false>, k_last_handover<2, 6, false>,
                                                                    k_last_handover<4, 6, false>, k_last_handover<8, 6, false>};
static decltype(&k_learn_scan_emit<1, 6>) lse_kernel(const Dev &d, int form, bool list = false) {
    if (list) return (form == LSE_TAB ? kt_lsel_tab : form == LSE_LARGE ? kt_lsel_large : kt_lsel_plain)[epl_slot(d)];
    return (form == LSE_TAB ? kt_lse_tab : form == LSE_LARGE ? kt_lse_large : kt_lse_plain)[epl_slot(d)];
}

// the form of k_learn_scan_emit this handle launches now (its occupancy is asked for at creation: size_launches)
static int lse_form(const htm_handle *h) { return scan_pool_is_large(h) ? LSE_LARGE : lean_tab(h->d) ? LSE_TAB : LSE_PLAIN; }

// the last launch of a step in the two- and three-launch schedules: learn(p) + scan(p) beside the select finish + winner list of the
// step of the other parity (n_emit blocks of it, or none)
// list: the step's first launch was k_first_handover -- the kernel with the list role, one block behind the scan's (it writes the
// step's winner list where that launch's block 0 did not, and resets its flag words: such a step ALWAYS ends in this form)
static void launch_learn_scan_emit(htm_handle *h, int p, int n_emit, bool list = false) {
    Dev &d = h->d;
    const int epl = learn_epl(d);
    const size_t lds = std::max(std::max(learn_lds(epl, 256), lean_scan_lds(d)), sizeof(EmitShared));
    // A large pool streams.  DYN (the default): the grid is what is resident at once and every block ends up scanning
    // (role_scan); the kernel is told by the sign of its n_scan argument.  More learning blocks than a small pool gets: a wave
    // per work item (a large learned pool has ~2 800 a step), so that no block joins late because its waves had second items.
    // BITHTM_SCAN_DYN=0: scan blocks with fixed shares -- more of them than are resident at once (as the select finish's and the
    // learning role's blocks leave, the dispatcher fills their slots; the 768 of the small-pool form left the launch 13 % longer).
    const bool large = scan_pool_is_large(h), dyn = large && h->knob.scan_dyn > 0;
    const int n_learn = dyn ? h->sz.lean_learn_blocks_large : h->sz.lean_learn_blocks;
    int n_scan = large ? h->sz.lean_scan_blocks_large : h->sz.lean_scan_blocks;
    if (dyn) n_scan = std::max(64, h->sz.lean_resident_large - n_emit - n_learn);
    const int grid = n_emit + n_learn + n_scan + (list ? 1 : 0);
    if (large && !dyn) n_scan = -n_scan;
    const int spec = dyn ? 0 : scan_spec_blocks(h);
    // (the launch's name says which form of the scan it holds: htm_profile_read is how tests and bench.py tell)
    const char *lse_name = large ? "tm_learn+tm_scan_large+sp_emit" : "tm_learn+tm_scan+sp_emit";
    LAUNCH_ON(h, h->stream, lds, lse_name, lse_kernel(d, lse_form(h), list), grid, 256, d, p, n_emit, n_learn, n_scan, spec);
}

// classification blocks of k_act_mid_rows (the two-launch schedule's first launch)
// (a large pool has a classification block read ~250 match words and classify tens of them: more blocks there, though they
// are not all resident from the start -- 350-pattern pool of the bench, 1.6 M segments: 32 blocks 11.7 k timesteps/s, 128: 13.3, 256: 13.3,
// 384: 13.1; three launches: 12.8)
static int lean2_classify_blocks(const htm_handle *h, int learning) {
    if (!learning) return 0;
    return scan_pool_is_large(h) && !h->knob.lean2_classify ? std::max(h->sz.lean2_classify_blocks, 192) : h->sz.lean2_classify_blocks;
}

// The two-launch schedule's first launch (k_act_mid_rows, htm_pipeline.h) for the step of parity p, its roles counted in the
// kernel's order.  n_overlap > 0: the coming step's overlap rides along (a steady-state step); else the duty cycle has blocks
// of its own (the last step of a call, a host-fed step).  The profile name and the LDS bytes are the call site's.
// handover: the batched run's form of the launch (k_first_handover, htm_handover.h: block 0 keeps its list in the dynamic LDS, so
// the launch asks for SEL_BINS * 4 bytes whether or not an overlap role rides along); else k_act_mid_rows
static void launch_act_mid_rows(htm_handle *h, const char *name, size_t lds, int p, int learning, const uint32_t *bank, int n_inputs, int n_overlap,
                                bool handover = false) {
    Dev &d = h->d;
    const int n_act = act_blocks(d), n_cls = lean2_classify_blocks(h, learning), n_rows = learning ? d.k : 0;
    const int n_duty = n_overlap ? 0 : h->sz.c256_blocks, n_clear = d.WPC * h->sz.c256_blocks;
    const int grid = n_act + 1 + n_cls + n_rows + n_overlap + n_duty + n_clear + h->sz.zero_blocks;
    if (handover)
        LAUNCH_ON(h, h->stream, std::max(lds, (size_t)SEL_BINS * 4), name, k_first_handover, grid, 256,
                  d, p, d.k, n_act, learning, n_cls, bank, n_inputs, n_rows, h->sz.G, n_overlap, n_duty, n_clear, h->knob.lean2_order, h->knob.handover_cap);
    else
        LAUNCH_ON(h, h->stream, lds, name, k_act_mid_rows, grid, 256,
                  d, p, d.k, n_act, learning, n_cls, bank, n_inputs, n_rows, h->sz.G, n_overlap, n_duty, n_clear, h->knob.lean2_order);
}

// sp_done: the winner list of this step exists (the previous step's last launch, or the cold start).  next_sp: select
// the next step's winners beside this step's Temporal Memory.
static void enqueue_lean(htm_handle *h, int p, int learning, const uint32_t *bank, int n_inputs, StepPlan plan) {
    Dev &d = h->d;
    if (h->knob.lean == 2) {                        // the two-launch schedule: both of these in one (htm_pipeline.h)
        launch_act_mid_rows(h, "tm_activate+tm_mid+sp_learn+sp_overlap", (size_t)SEL_BINS * 4, p, learning, bank, n_inputs,
                            plan.next_sp ? h->sz.lean2_overlap_blocks : 0, true);
    } else {
        const int n_act = act_blocks(d), n_rows = learning ? d.k : 0;
        const int n_cls = learning ? kClassifyBlocks : 0, n_ov = plan.next_sp ? h->sz.lean_overlap_blocks : 0;
        LAUNCH(h, "tm_activate+sp_learn", k_act_rows, n_act + n_rows + (1 + d.WPC) * h->sz.c256_blocks, 256, d, p, d.k, n_act, bank, n_inputs, n_rows, h->sz.c256_blocks);
        LAUNCH_ON(h, h->stream, (size_t)SEL_BINS * 4, "tm_mid+sp_overlap", k_mid_overlap, 1 + n_cls + n_ov + h->sz.zero_blocks, 256, d, p, d.k, 1, learning, n_cls,
                  bank, n_inputs, h->sz.G, n_ov);
    }
    launch_learn_scan_emit(h, p, plan.next_sp ? h->sz.c256_blocks : 0, h->knob.lean == 2);
}

static decltype(&k_learn_overlap<1>) const kt_learn_overlap[4] = {k_learn_overlap<1>, k_learn_overlap<2>, k_learn_overlap<4>, k_learn_overlap<8>};
static decltype(&k_scan_sel<true, 1>) const kt_scan_sel[4] = {k_scan_sel<true, 1>, k_scan_sel<false, 1>, k_scan_sel<true, 6>, k_scan_sel<false, 6>};

// the four launches of a pipelined step (see the kernels): step p's Temporal Memory beside SP work of
// the following steps
static void enqueue_pipelined(htm_handle *h, int p, int learning, const uint32_t *bank, int n_inputs, StepPlan plan) {
    Dev &d = h->d;
    const int n_cls = learning ? kClassifyBlocks : 0;
    const int n_emit = plan.next_sp ? h->sz.c256_blocks : 0;
    LAUNCH_ON(h, h->stream, sizeof(EmitShared), "tm_activate+sp_emit", k_open_emit, n_emit + act_blocks(d), 256, d, p, n_emit, d.k);
    const int n_rows = (plan.next_sp && learning) ? d.k : 0, n_duty = plan.next_sp ? h->sz.c256_blocks : 0;
    LAUNCH(h, "tm_mid+sp_learn", k_mid_rows, 1 + n_cls + n_rows + n_duty + h->sz.zero_blocks, 256, d, p, d.k, 1, learning, n_cls, bank, n_inputs, n_rows, 1, n_duty);
    // (the front is that of step + 2: same parity as this step)
    LAUNCH_ON(h, h->stream, std::max(learn_lds(learn_epl(d)), (size_t)SEL_BINS * 4), "tm_learn+sp_overlap", kt_learn_overlap[epl_slot(d)],
              kLearnBlocks + (plan.next_front ? h->sz.sp_blocks : 0), RB, d, p, kLearnBlocks, bank, n_inputs, h->sz.G, p, 2);
    const bool use_lds = bitmap_fits_lds(d), large = scan_pool_is_large(h);
    const int n_sel = plan.next_front ? 64 : 0, n_clear = plan.next_sp ? h->sz.c256_blocks : 0;
    LAUNCH_ON(h, h->stream, std::max(scan_lds(d, use_lds), sizeof(SelShared)), large ? "tm_scan_large+sp_select" : "tm_scan+sp_select",
              kt_scan_sel[scan_slot(large, use_lds)], h->sz.scan_blocks + n_sel + n_clear, 256, d, p, n_sel, n_clear, p, scan_spec_blocks(h));
}

// work of a step that is not captured in its graph: the first step of a pipelined run has no SP work
// done for it; run the SP's step on its own, and the front of the next one
static void enqueue_cold_start(htm_handle *h, const uint32_t *bank, int n_inputs, int learning, StepPlan plan) {
    Dev &d = h->d;
    const int p = (int)(h->step_host & 1);
    if (plan.sp_done || !plan.next_sp) return;
    const int wmode = step_wmode(h);
    if (can_lean(h)) {                              // the winner list of this step, nothing else
        enqueue_sp_front(h, bank, n_inputs, p, wmode);
        enqueue_sp_back(h, bank, n_inputs, p, 1, 0, false, wmode);
        return;
    }
    enqueue_sp_front(h, bank, n_inputs, p, wmode);
    enqueue_sp_back(h, bank, n_inputs, p, 1, EMIT_DUTY | EMIT_CLEAR, learning != 0, wmode);
    LAUNCH(h, "sp_overlap", k_sp_overlap, h->sz.sp_blocks, RB, d, bank, n_inputs, h->sz.G, p, p ^ 1, 1, 0);
    LAUNCH(h, "sp_select", k_sel_pass, h->sz.sel_blocks, RB, d, 1, p ^ 1);
}

// grid of the reset launch (htm_reset.h): a grid-stride pass over the cell words and per-cell maxima
static int reset_blocks(const Dev &d) { return std::max(1, std::min(1024, (d.C * d.KP + 255) / 256)); }

// in a run with reset bits: the reset of the step of parity p if its bank row asks for one (before its activation role)
static void enqueue_run_reset(htm_handle *h, RunModes m, int p) {
    if (m.resetting) LAUNCH(h, "tm_reset", k_tm_reset, reset_blocks(h->d), 256, h->d, p, h->d_reset, m.recording ? h->d_rec : nullptr, 0u);
}

static void enqueue_rest(htm_handle *h, RunModes m, int p, const uint32_t *bank, int n_inputs, int learning, StepPlan plan) {
    enqueue_run_reset(h, m, p);
    if ((plan.sp_done || plan.next_sp) && can_lean(h)) {
        enqueue_lean(h, p, learning, bank, n_inputs, plan);
    } else if (plan.sp_done || plan.next_sp) {
        enqueue_pipelined(h, p, learning, bank, n_inputs, plan);
    } else {                                        // one role per launch
        enqueue_sp_back(h, bank, n_inputs, p, 1, EMIT_ALL, false, step_wmode(h));
        enqueue_tm(h, h->d.k, learning, 1, p, bank, n_inputs, true);
    }
}

// grid of the capture launch: a thread per pair of the step's row
static int cap_blocks(const Dev &d) { return std::max(1, (d.k * d.WPC + 255) / 256); }

// grid of the record launches (htm_record.h): REC_BLOCKS_MIN, or more where the winner list needs a thread per entry
static int rec_blocks(const Dev &d) { return std::max(REC_BLOCKS_MIN, (d.k + 255) / 256); }

// the record of the step of parity p, behind its last launch (htm_record.h); nothing outside a recorded call
static void enqueue_record(htm_handle *h, RunModes m, int p) {
    if (m.recording) LAUNCH(h, "record", k_rec_step, rec_blocks(h->d), 256, h->d, p, h->d_rec);
}

// the predicted-input votes of the step of parity p, behind its last launch (htm_decode.h); nothing outside a decoding call
static void enqueue_decode(htm_handle *h, RunModes m, int p) {
    if (m.decoding) LAUNCH(h, "predicted_input", k_pin_step, pin_blocks(h->d.C), 256, h->d, p, (const PinDev *)h->d_pin);
}

// The four-launch schedule applies the permanence rows of step t + 1 inside step t (k_mid_rows, rows_ahead = 1), before step t's
// scan has set its predictions: behind that scan the mask is no longer the one the votes of step t are taken on.  A decoding
// call of such a handle runs unpipelined (every other schedule applies the rows of step t within step t).
static bool decode_unpipelined(const htm_handle *h) { return h->pin_out && !can_lean(h); }

// Run feedback (htm_forecast.h): behind the step of parity p, the votes of the state it leaves into the scratch row, then the
// bank row the next step reads.  That step's overlap must come behind these two launches: a feeding call runs unpipelined.
static void enqueue_feed(htm_handle *h, RunModes m, int p) {
    if (!m.feeding) return;
    LAUNCH(h, "feedback_votes", k_feed_votes, pin_blocks(h->d.C), 256, h->d, p, (const FeedDev *)h->d_feed);
    LAUNCH(h, "feedback_encode", k_feed_step, 1, ENC_THREADS, h->d, p, (const FeedDev *)h->d_feed);
}

// grid of the launch that zeroes a decoding call's n x I votes (grid-stride)
static int pin_begin_blocks(int n, int I) { return (int)std::max<size_t>(1, std::min<size_t>(1024, ((size_t)n * I + 255) / 256)); }

// the active-cell words of the step of parity p, directly behind its record launch (htm_classifier.h); nothing outside a capturing call
static void enqueue_capture(htm_handle *h, RunModes m, int p) {
    if (m.capturing) LAUNCH(h, "active_cells", kcls_capture, cap_blocks(h->d), 256, h->d, p, (const RecDev *)h->d_rec, (const ClsCapDev *)h->d_cap);
}

// everything behind a step's own launches that the call's modes ask for
static void enqueue_step_outputs(htm_handle *h, RunModes m, int p) {
    enqueue_record(h, m, p);
    enqueue_capture(h, m, p);
    enqueue_decode(h, m, p);
    enqueue_feed(h, m, p);
}

static int enqueue_step(htm_handle *h, RunModes m, const uint32_t *bank, int n_inputs, int learning, StepPlan plan, const uint32_t *host_input = nullptr) {
    const int p = (int)(h->step_host & 1);
    if (!plan.sp_done && !plan.next_sp) enqueue_sp_front(h, bank, n_inputs, p, step_wmode(h), host_input);
    enqueue_cold_start(h, bank, n_inputs, learning, plan);
    enqueue_rest(h, m, p, bank, n_inputs, learning, plan);
    enqueue_step_outputs(h, m, p);
    h->step_host += 1;
    return launch_status(h->err);
}

extern "C" int htm_abi_version(void) { return BITHTM_ABI_VERSION; }

extern "C" const char *htm_last_error(const htm_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

extern "C" void htm_destroy(htm_handle *h) {
    if (!h) return;
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        g_registry.erase(std::remove(g_registry.begin(), g_registry.end(), h), g_registry.end());
    }
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    for (auto &kv : h->graphs) hipGraphExecDestroy(kv.second);
    for (auto &kv : h->shard_graphs) hipGraphExecDestroy(kv.second);
    for (auto &kv : h->tm_graphs) hipGraphExecDestroy(kv.second);
    for (auto &kv : h->sp_graphs) hipGraphExecDestroy(kv.second);
    for (auto &v : h->prof_events)
        for (auto &pr : v) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (hipEvent_t e : h->prof_all) hipEventDestroy(e);
    if (h->rccl_comm && g_rccl_destroy) g_rccl_destroy(h->rccl_comm);
    for (void *p : h->allocs) hipFree(p);
    for (void *p : h->weight_allocs) hipFree(p);
    if (h->seg_pinned) hipHostFree(h->seg_pinned);
    if (h->own_stream) hipStreamDestroy(h->stream);
    if (HtmShared *sh = h->shared) {              // the last of a parent and its views frees the weights (and the parent's stream)
        bool last;
        {
            std::lock_guard<std::mutex> lock(g_shared_mutex);
            if (sh->parent == h) sh->parent = nullptr;
            last = --sh->refs == 0;
        }
        if (last) {
            for (void *p : sh->allocs) hipFree(p);
            if (sh->own_stream) hipStreamDestroy(sh->stream);
            delete sh;
        }
    }
    delete h;
}

static int fail_create(htm_handle *h, const std::string &msg, int code) {
    g_create_error = msg;
    if (h) { h->err = msg; htm_destroy(h); }
    return code;
}

// The device state of a handle in two parts.  The weights -- what learning changes and an inference view aliases (htm_create_view):
// the SP permanences and connected mask, the segment store.
static int alloc_weights(htm_handle *h) {
    Dev &d = h->d;
    const htm_config *cfg = &h->cfg;
    const size_t C = d.C;
    int rc = 0;
    if (cfg->enable_sp) {
        rc |= dalloc_weights(h, &d.perm, C * d.Ipad);
        rc |= dalloc_weights(h, &d.mask, C * d.W);
        // the mask again, by byte position (d.planes: the two-launch schedule's overlap reads the planes of the input's non-zero
        // bytes only); zeroed like the mask, and a view aliases it like the mask.  A shard has none.
        d.plane_stride = (d.C + 255) & ~255;
        // (... whose mask words count in 32 bits: plane_diff_store_late takes a row's number from its address)
        if (h->world == 1 && C * d.W < ((size_t)1 << 32)) rc |= dalloc_weights(h, &d.planes, (size_t)4 * d.W * d.plane_stride);
    }
    if (cfg->enable_tm) {
        const size_t S = d.Lcap, E = d.E, KP = d.KP;
        rc |= dalloc_weights(h, &d.seg_cell, S);
        rc |= dalloc_weights(h, &d.seg_nsyn, S);
        rc |= dalloc_weights(h, &d.presyn, S * E);
        rc |= dalloc_weights(h, &d.sperm, S * E);
        rc |= dalloc_weights(h, &d.segcount, C * KP);
    }
    return rc;
}

// ... and everything one input stream carries from step to step (a view owns its own)
static int alloc_stream_state(htm_handle *h) {
    Dev &d = h->d;
    const htm_config *cfg = &h->cfg;
    const int world = h->world;
    int rc = 0;
    const size_t C = d.C, k = d.k;
    rc |= dalloc(h, &d.ctr, 1);
    rc |= dalloc(h, &d.active_cols[0], k + 8);     // (+8: the TM's list pass reads 8 entries per thread)
    rc |= dalloc(h, &d.active_cols[1], k + 8);
    if (cfg->enable_sp) {
        rc |= dalloc(h, &d.duty, C);
        for (int q = 0; q < 2; ++q) {
            rc |= dalloc(h, &d.overlap[q], C);
            rc |= dalloc(h, &d.boosted[q], C);
            rc |= dalloc(h, &d.key[q], C);
        }
        rc |= dalloc(h, &d.hist, (size_t)2 * SEL_MAX_PASSES * SEL_BINS);
        rc |= dalloc(h, &d.hist0, (size_t)2 * HIST0_PAR);
        rc |= dalloc(h, &d.sel_blk, (C + 255) / 256);
        rc |= dalloc(h, &d.sel_rec, (C + 255) / 256 * 32);
        rc |= dalloc(h, &d.input_stage, (size_t)d.W);
    }
    if (cfg->enable_tm) {
        const size_t S = d.Lcap, G = d.Scap;        // local rows (= ids on an unsharded handle), segment ids
        const size_t KP = d.KP, WPC = d.WPC;
        for (int q = 0; q < 2; ++q) {
            rc |= dalloc(h, &d.act[q], C * WPC);
            rc |= dalloc(h, &d.pred[q], C * WPC);
            rc |= dalloc(h, &d.winners[q], k * KP);
        }
        rc |= dalloc(h, &d.win[0], C * WPC);
        rc |= dalloc(h, &d.win[1], C * WPC);
        d.colwords = (int)((C + 63) / 64) * 2;
        // (the emit blocks write the bitmap words of whole 256-column blocks)
        const size_t colwords_padded = (size_t)((C + 255) / 256) * 8;
        rc |= dalloc(h, &d.colbits[0], colwords_padded);
        rc |= dalloc(h, &d.colbits[1], colwords_padded);
        rc |= dalloc(h, &d.bursting, k);
        rc |= dalloc(h, &d.actw_id, k * WPC + 8);
        rc |= dalloc(h, &d.winw_idx, k * WPC + 8);
        rc |= dalloc(h, &d.actcnt, k * WPC + 8);
        rc |= dalloc(h, &d.act_list, k * WPC + 16);   // (staged into LDS in 16-byte units)
        rc |= dalloc(h, &d.col_rank[0], colwords_padded);
        rc |= dalloc(h, &d.col_rank[1], colwords_padded);
        rc |= dalloc(h, &d.unacc_word, k * WPC + 8);
        rc |= dalloc(h, &d.fan, (size_t)2 * FAN_COUNTERS * FAN_STRIDE);
        rc |= dalloc(h, &d.unacc_list, k * KP);
        for (int q = 0; q < 2; ++q) {
            rc |= dalloc(h, &d.cellmax[q], C * KP);
            rc |= dalloc(h, &d.match_bits[q], (S + 255) / 256 * 8);
        }
        rc |= dalloc(h, &d.seg_info, S);
        rc |= dalloc(h, &d.seg_jit, S);
        // (the learning role's own buffers: a view, which never learns, keeps them too -- its kernels are the parent's, and
        // none of them is told that a buffer is missing)
        rc |= dalloc(h, &d.work, (size_t)d.work_cap);
        rc |= dalloc(h, &d.recyc_cnt, (G + 1023) / 1024);
        rc |= dalloc(h, &d.recyc_cnt2, ((G + 1023) / 1024 + 1023) / 1024 + 1);
        rc |= dalloc(h, &d.recyc_need, 2 * k * KP);
        rc |= dalloc(h, &d.dead_list, (size_t)1 + DEAD_CAP);
        if (world > 1) {
            rc |= dalloc(h, &d.seg_gid, S);
            rc |= dalloc(h, &d.g2l, G);
            rc |= dalloc(h, &d.dead_bits, (G + 31) / 32 + 32);
            rc |= dalloc(h, &d.lfree, S);
            rc |= dalloc(h, &d.asg_gid, k * 32);
            rc |= dalloc(h, &d.cand_cols, (size_t)d.n_cand + 8);
            if (!rc && (hipMemsetAsync(d.seg_gid, 0xFF, S * 4, h->stream) != hipSuccess ||
                        hipMemsetAsync(d.g2l, 0xFF, G * 4, h->stream) != hipSuccess)) { h->err = "hipMemsetAsync failed"; rc = HTM_ERR_HIP; }
        }
        rc |= dalloc(h, &h->d_cols_stage, k);
    }
    if (h->knob.trace) rc |= dalloc(h, &d.trace, (size_t)8 * 4096 * 2);
    return rc;
}

// The environment, read here only: a knob's text, or an integer knob -- dflt when it is not given, else its value clamped to
// [lo, hi] -- or a flag (a given value is on unless it reads 0)
static const char *env_str(const char *name) { return getenv(name); }
static int env_int(const char *name, int dflt, int lo = INT_MIN, int hi = INT_MAX) {
    const char *e = env_str(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}
static int env_flag(const char *name, int dflt) {
    const char *e = env_str(name);
    return e ? atoi(e) != 0 : dflt;
}

static Knobs read_knobs() {
    Knobs k;
    k.graph_steps = env_int("BITHTM_GRAPH_STEPS", 16, 1, 256);
    k.eager_below = env_int("BITHTM_EAGER_BELOW", 64, 0);
    k.trace = env_str("BITHTM_TRACE") != nullptr;
    const char *until = env_str("BITHTM_TRACE_UNTIL");
    k.trace_until = until ? (uint32_t)strtoul(until, nullptr, 10) : 0xFFFFFFFFu;
    k.lean = env_int("BITHTM_LEAN", 2, 0, 2);
    k.lean2_classify = env_int("BITHTM_LEAN2_CLASSIFY", 0, 1);
    // the host-fed step (htm_step): select finish alone + k_act_mid_rows, instead of select finish with the activation in its blocks +
    // k_mid_rows (BITHTM_STEP_SPLIT=0: as before)
    k.step_split = env_flag("BITHTM_STEP_SPLIT", 1);
    {   // the grid order of k_act_mid_rows' roles (hex digits: 0 activation, 1 middle, 2 rows, 3 overlap); a permutation with 0 before 1
        // (measured at the bench shape, 8 waves per SIMD: 0312 42.4 k timesteps/s, 0321 41.9, 0123 41.2, 3201 40.2)
        const char *e = env_str("BITHTM_LEAN2_ORDER");
        const int o = e ? (int)strtol(e, nullptr, 16) : 0x0312;
        int seen = 0, pos[4] = {-1, -1, -1, -1};
        for (int i = 0; i < 4; ++i) { const int r = (o >> (4 * (3 - i))) & 15; if (r < 4) { seen |= 1 << r; pos[r] = i; } }
        k.lean2_order = (o >= 0 && o <= 0x3333 && seen == 15 && pos[0] < pos[1]) ? o : 0x0312;
    }
    k.fuse_tm = env_flag("BITHTM_FUSE_TM", 1);
    k.shard_window = env_flag("BITHTM_SHARD_WINDOW", 1);
    k.scan_large = env_int("BITHTM_SCAN_LARGE", -1);
    // (test knob: a small model crosses the threshold in the middle of a run, as the headline shape does with more patterns)
    k.scan_large_above = env_int("BITHTM_SCAN_LARGE_ABOVE", 3 * 1536 * SCAN_SEGS, 0);
    k.step_window = env_flag("BITHTM_STEP_WINDOW", 1);
    k.tail_rows = env_flag("BITHTM_TAIL_ROWS", 1);
    // (0: scan blocks with fixed shares, nothing joining; else every block of the launch joins the scan)
    k.scan_dyn = env_flag("BITHTM_SCAN_DYN", 1);
    k.defer_tail = env_flag("BITHTM_DEFER_TAIL", 1);
    // groups of inference views: 1 = one scan of the shared store for up to M members at a time; 0 (the default: at the bench shape it
    // reads 6.4 times fewer bytes than the per-member scans yet takes 2.6 times longer) = a scan per member;
    // and a cap of M (test knob: several member chunks at small shapes)
    k.shared_scan = env_flag("BITHTM_SHARED_SCAN", 0);
    k.shared_members = env_int("BITHTM_SHARED_SCAN_MEMBERS", 0, 0);
    k.lean_overlap = env_int("BITHTM_LEAN_OVERLAP", 0, 1);
    k.lean_learn = env_int("BITHTM_LEAN_LEARN", 0, 1);
    k.lean_learn_large = env_int("BITHTM_LEAN_LEARN_LARGE", 0, 1);
    k.lean_scan = env_int("BITHTM_LEAN_SCAN", 0, 1);
    k.lean_scan_large = env_int("BITHTM_LEAN_SCAN_LARGE", 0, 1);
    k.scan_blocks = env_int("BITHTM_SCAN_BLOCKS", 0, 1);
    // test knobs: more launched digits (smaller buckets); fewer record slots (forces the fallback)
    k.sel_launch_digits = env_int("BITHTM_SEL_LAUNCH_DIGITS", -1, 0);
    k.cand_d = env_int("BITHTM_CAND_D", CAND_D, 0, CAND_D);
    k.cand_pairwise = env_int("BITHTM_CAND_PAIRWISE", CAND_PAIRWISE, 0);
    k.cls_rows_max = env_int("BITHTM_CLASSIFY_WORDS_ABOVE", -1, 0);
    // (test knob: entries of the list of winners without a segment that block 0 of k_first_handover keeps in LDS; the rest goes through memory)
    k.handover_cap = env_int("BITHTM_HANDOVER_LDS_CAP", HANDOVER_LIST_MAX, 0, HANDOVER_LIST_MAX);
    k.win_offset = env_int("BITHTM_SEL_WINDOW_OFFSET", 0, 0);
    k.cand_zoom = env_int("BITHTM_CAND_ZOOM", -1);      // (the pairs above which a merge is cut to a sub-bin; -1 = more pairs than blocks by a quarter)
    k.cand_speculate = env_flag("BITHTM_CAND_SPECULATE", 1);     // (0 = always the general path)
    k.cand_take_all = env_flag("BITHTM_CAND_TAKE_ALL", 1);       // (0 = a shard's local select always cuts exactly)
    k.poll_delay = env_int("BITHTM_POLL_DELAY", 7, 0, 64);      // (the select finish's first look at the other blocks' records: x 256 clocks after its own)
    k.cand_others = env_int("BITHTM_CAND_OTHERS", CAND_OTHERS, 0, CAND_OTHERS);
    return k;
}

// The launch sizes of a new handle (h->sz, and the select's digits in its Dev): from its shape, its knobs and what the runtime
// says is resident at once on the device
static void size_launches(htm_handle *h) {
    Dev &d = h->d;
    const Knobs &k = h->knob;
    Sizes &z = h->sz;
    // lanes per SP row: the smallest power of two >= W4, at most 64
    z.G = 1;
    while (z.G < d.W4 && z.G < 64) z.G <<= 1;
    // few fat blocks for the kernels that flush a histogram: every block adds into the same few
    // hot bins and same-address global atomics are slow (~88 per us per address)
    const int rows_per_block = (RB / 64) * 4 * (64 / z.G);   // waves x 4 row groups in flight
    z.sp_blocks = std::max(1, std::min((d.c1 - d.c0 + rows_per_block - 1) / rows_per_block, 256));
    z.sel_blocks = std::max(1, std::min((d.sel_hi - d.sel_lo + RB - 1) / RB, 128));
    z.c256_blocks = (d.sel_hi - d.sel_lo + 255) / 256;        // blocks of the emit role: 256 columns of the select's range each
    z.s1024_blocks = std::max(1, (d.Scap + 1023) / 1024);
    z.scan_blocks = std::max(1, std::min((d.Lcap + SCAN_SEGS - 1) / SCAN_SEGS, 2048));
    if (z.scan_blocks > 256) z.scan_blocks = (z.scan_blocks + 255) & ~255;     // (role_scan: whole groups of 256 blocks)
    z.zero_blocks = std::max(1, std::min((d.Lcap / 128 + 4095) / 4096, 1024));     // k_mid_rows: 16 stores of 16 bytes per thread at most
    // the three-launch schedule: waves of one 256-thread block per work item in the steady state; the scan's waves take
    // two groups of segments each, so that emit + learn + scan are all resident at once (tuning knobs)
    z.lean_overlap_blocks = k.lean_overlap ? k.lean_overlap : z.sp_blocks * (RB / 256);
    z.lean2_overlap_blocks = d.planes ? (d.c1 - d.c0 + 255) / 256 : z.lean_overlap_blocks;
    z.lean_learn_blocks = k.lean_learn ? k.lean_learn : 512;
    z.lean_learn_blocks_large = k.lean_learn_large ? k.lean_learn_large : k.lean_learn ? z.lean_learn_blocks : 768;
    z.lean_scan_blocks = k.lean_scan ? k.lean_scan : (z.scan_blocks > 512 ? std::max(256, (z.scan_blocks * 3 / 8 + 255) & ~255) : z.scan_blocks);
    z.lean_scan_blocks_large = k.lean_scan_large ? k.lean_scan_large : k.lean_scan ? z.lean_scan_blocks : z.scan_blocks;
    if (k.scan_blocks) z.scan_blocks = k.scan_blocks;      // (tuning knob: the defaults above stay)
    hipDeviceProp_t prop;
    const bool have_prop = hipGetDeviceProperties(&prop, h->device) == hipSuccess;
    z.cus = have_prop ? prop.multiProcessorCount : 256;
    // boosted = float32 factor x integer overlap <= input_dim has at most 24 + bit_length(I)
    // significant bits, so the low 53 - 24 - bit_length(I) bits of every key are zero and the
    // radix passes that would only see them are skipped.
    int B = 0;
    while ((1ll << B) <= (long long)d.I) ++B;
    const int informative = std::min(64, 64 - (29 - B) - KEY_SHIFT);      // (select_key moves the bits up by KEY_SHIFT)
    d.sel_passes = std::max(1, std::min(SEL_MAX_PASSES, (informative + SEL_DIGIT - 1) / SEL_DIGIT));
    d.low_zero = 64 - informative;            // key bits [0, low_zero) are zero in every key
    // Emit grids whose blocks are all resident at once finish the select inside k_sp_emit (two digits
    // by launches, the rest through the record exchange, in which blocks wait for each other).  What
    // fits is asked of the runtime, kernel by kernel, not assumed.
    int per_cu_emit = 0, per_cu_open = 0;
    if (have_prop && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_emit, (const void *)k_sp_emit, 256, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_open, (const void *)k_open_emit, 256, sizeof(EmitShared)) == hipSuccess) {
        z.emit_fits = z.c256_blocks <= std::min(1024, per_cu_emit * z.cus);
        // the pipelined launch puts the activation blocks of the current step behind the emit blocks
        z.emit_fits_open = z.emit_fits && z.c256_blocks + act_blocks(d) <= std::min(1024, per_cu_open * z.cus);
        // the three-launch schedule: the emit blocks come first in the grid of the learn + scan + emit kernel
        // (asked of every form launch_learn_scan_emit may launch for this handle -- LDS tables or not, small-pool or
        // large-pool scan: they differ in launch bounds and registers -- and the smallest answer counts)
        int per_cu_lean = 1 << 30;
        z.lean_resident_large = 1 << 30;
        const size_t lean_lds = std::max(std::max(learn_lds(learn_epl(d), 256), lean_scan_lds(d)), sizeof(EmitShared));
        bool asked = h->cfg.enable_tm && z.emit_fits && lean_lds <= 64 * 1024;
        for (int form = LSE_TAB; asked && form <= LSE_LARGE; ++form) {
            if (form == LSE_TAB && !lean_tab(d)) continue;           // (never launched without the tables)
            int per_cu = 0;
            int per_cu_list = 0;                      // (the batched run's form of the launch, with the list role: the same figures)
            asked = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)lse_kernel(d, form), 256, lean_lds) == hipSuccess &&
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_list, (const void *)lse_kernel(d, form, true), 256, lean_lds) == hipSuccess;
            per_cu = std::min(per_cu, per_cu_list);
            per_cu_lean = std::min(per_cu_lean, per_cu);
            if (asked && form == LSE_LARGE) z.lean_resident_large = per_cu * z.cus;
        }
        z.emit_fits_lean = asked && z.c256_blocks <= std::min(1024, per_cu_lean * z.cus);
        if (z.lean_resident_large == (1 << 30)) z.lean_resident_large = 4 * z.cus;
    } else {
        (void)hipGetLastError();
        z.emit_fits = z.emit_fits_open = z.emit_fits_lean = false;
        z.lean_resident_large = 1024;
    }
    if (k.lean2_classify) {
        z.lean2_classify_blocks = k.lean2_classify;
    } else {
        // the two-launch schedule's first launch: as many classification blocks as are resident BESIDE the activation, the
        // overlap and the winner rows -- a block that waits for a slot starts a round late, and the middle role's blocks wait for
        // the activation whenever they start (bench shape: 164 + 512 + 1 311 + 1 of 2 048 slots leave 60; small models get 384)
        int per_cu = 0, resident = 1536;
        int per_cu_run = 0;                           // (the batched run's form of the launch, k_first_handover: the same 8 blocks per CU)
        if (have_prop && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)k_act_mid_rows, 256, (size_t)SEL_BINS * 4) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_run, (const void *)k_first_handover, 256, (size_t)SEL_BINS * 4) == hipSuccess)
            resident = std::min(per_cu, per_cu_run) * z.cus;
        else
            (void)hipGetLastError();
        // (the overlap counted as the column-major role's blocks, also where the launch's own role reads the byte planes and takes
        // half as many: the slots that role frees are not the classification's to fill -- its blocks poll the fan-in beside the
        // rows.  Measured at the bench shape with the plane role, 316 free slots: 32 blocks 46.2 k timesteps/s, 64: 45.7, 128:
        // 45.3, 312: 42.7 -- so every shape keeps the count it had)
        const int others = act_blocks(d) + z.lean_overlap_blocks + d.k + 1;
        // (... but no more than 32 where they leave fewer than 128: measured at the bench shape, 60 free slots -- 32 blocks 42.4 k
        // timesteps/s, 40: 41.9, 56: 41.6)
        const int room = (resident - others) & ~7;
        z.lean2_classify_blocks = room >= 128 ? std::min(kClassifyBlocks, room) : 32;
    }
    z.sel_passes_full = d.sel_passes;
    z.sel_passes_fused = std::min(d.sel_passes, 2);
    if (k.sel_launch_digits >= 0) z.sel_passes_fused = std::max(2, std::min(d.sel_passes, k.sel_launch_digits));
}

extern "C" int htm_create(const htm_config *cfg, htm_handle **out) {
    if (!cfg || !out) return fail_create(nullptr, "htm_create: null argument", HTM_ERR_ARGUMENT);
    if (cfg->struct_bytes != sizeof(htm_config)) return fail_create(nullptr, "htm_create: htm_config size mismatch (ABI)", HTM_ERR_ARGUMENT);
    if (cfg->column_dim < 1 || cfg->active_columns < 1 || cfg->active_columns > cfg->column_dim)
        return fail_create(nullptr, "htm_create: need 1 <= active_columns <= column_dim", HTM_ERR_ARGUMENT);
    if (cfg->enable_sp && cfg->input_dim < 1) return fail_create(nullptr, "htm_create: input_dim < 1", HTM_ERR_ARGUMENT);
    if (cfg->enable_tm) {
        if (cfg->cell_dim < 1 || cfg->cell_dim > 64) return fail_create(nullptr, "htm_create: cell_dim must be in 1..64", HTM_ERR_ARGUMENT);
        if (cfg->segment_slots < 64 || cfg->segment_slots > MAX_SLOTS || cfg->segment_slots % 64)
            return fail_create(nullptr, "htm_create: segment_slots must be a multiple of 64 in 64..512", HTM_ERR_ARGUMENT);
        if (cfg->segment_capacity < 1) return fail_create(nullptr, "htm_create: segment_capacity < 1", HTM_ERR_ARGUMENT);
        if (cfg->segment_sampling_synapses < 1 || cfg->segment_sampling_synapses > 64)
            return fail_create(nullptr, "htm_create: segment_sampling_synapses must be in 1..64", HTM_ERR_ARGUMENT);
        if (cfg->segment_activation_threshold < cfg->segment_matching_threshold)      // projections.py:211
            return fail_create(nullptr, "htm_create: activation threshold < matching threshold", HTM_ERR_ARGUMENT);
        if ((long long)cfg->column_dim * (cfg->cell_dim > 32 ? 64 : 32) > 0x7FFFFFFFLL) return fail_create(nullptr, "htm_create: column_dim too large", HTM_ERR_ARGUMENT);
    }
    if (!cfg->enable_sp && !cfg->enable_tm) return fail_create(nullptr, "htm_create: nothing enabled", HTM_ERR_ARGUMENT);
    const int world = cfg->shard_world > 1 ? cfg->shard_world : 1;
    if (world > 1) {
        if (!cfg->enable_sp || !cfg->enable_tm) return fail_create(nullptr, "htm_create: a sharded handle needs SP and TM", HTM_ERR_ARGUMENT);
        if (cfg->cell_dim > 32) return fail_create(nullptr, "htm_create: a sharded handle takes cell_dim up to 32 (the exchange record carries one 32-bit word per column)", HTM_ERR_ARGUMENT);
        if (world > 64) return fail_create(nullptr, "htm_create: at most 64 shards", HTM_ERR_ARGUMENT);
        if (cfg->shard_rank < 0 || cfg->shard_rank >= world) return fail_create(nullptr, "htm_create: shard_rank out of range", HTM_ERR_ARGUMENT);
        if (cfg->column_dim % (world * 64)) return fail_create(nullptr, "htm_create: column_dim must be a multiple of 64 * shard_world", HTM_ERR_ARGUMENT);
    }

    htm_handle *h = new htm_handle();
    h->cfg = *cfg;
    h->device = cfg->device;
    h->rank = world > 1 ? cfg->shard_rank : 0;
    h->world = world;
    h->knob = read_knobs();
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail_create(h, std::string("hipSetDevice: ") + hipGetErrorString(e), HTM_ERR_HIP);
    if (cfg->use_caller_stream) {
        h->stream = (hipStream_t)cfg->stream;          // NULL = the default stream
    } else {
        e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
        if (e != hipSuccess) return fail_create(h, std::string("hipStreamCreate: ") + hipGetErrorString(e), HTM_ERR_HIP);
        h->own_stream = true;
    }
    Dev &d = h->d;
    d.I = cfg->enable_sp ? cfg->input_dim : 0;
    d.W = ((d.I + 127) / 128) * 4;
    d.W4 = d.W / 4;
    d.Ipad = d.W * 32;
    d.C = cfg->column_dim;
    d.world = world;
    d.c0 = h->rank * (d.C / world);
    d.c1 = d.c0 + d.C / world;
    d.K = cfg->enable_tm ? cfg->cell_dim : 0;
    d.KP = d.K > 32 ? 64 : 32;
    d.LK = d.K > 32 ? 6 : 5;
    d.WPC = d.KP / 32;
    d.k = cfg->active_columns;
    d.E = cfg->enable_tm ? cfg->segment_slots : 64;
    d.Scap = cfg->enable_tm ? cfg->segment_capacity : 0;
    d.Lcap = d.Scap;
    if (world > 1) {
        const long long dflt = std::min<long long>(d.Scap, 2LL * d.Scap / world + 1024);
        d.Lcap = cfg->segment_capacity_local > 0 ? std::min(cfg->segment_capacity_local, cfg->segment_capacity) : (int)dflt;
    }
    d.work_cap = d.Lcap + d.k * d.KP;
    // the select: all columns and their k largest; a shard selects its own candidates for the exchange
    d.sel_lo = d.c0; d.sel_hi = d.c1;
    d.sel_k = d.n_cand = std::min(d.k, d.c1 - d.c0);
    d.cand_cap = shard_cand_cap(d.n_cand, d.c1 - d.c0);
    d.hot_budget = std::max(1, std::min(d.cand_cap, (SHARD_HOT_KEYS * 1024) / std::max(world, 1)));
    d.hot_target = std::max(1, std::min(d.sel_k, d.hot_budget / 2));
    d.sp_thr = cfg->sp_permanence_threshold; d.sp_don = cfg->sp_delta_on; d.sp_doff = cfg->sp_delta_off;
    d.coef = cfg->boost_coefficient; d.mom = cfg->duty_momentum; d.dinc = cfg->duty_increment;
    d.lrn_act = cfg->tm_learn_active; d.lrn_inact = cfg->tm_learn_inactive;
    d.pun_act = cfg->tm_punish_active; d.pun_inact = cfg->tm_punish_inactive;
    d.lrn_prune = cfg->tm_learn_prune; d.pun_prune = cfg->tm_punish_prune;
    d.perm_init = cfg->tm_permanence_initial; d.perm_thr = cfg->tm_permanence_threshold;
    d.eps = EPS32;
    d.act_thr = cfg->segment_activation_threshold; d.match_thr = cfg->segment_matching_threshold;
    d.sample = cfg->segment_sampling_synapses;
    d.seed = cfg->seed;
    const Knobs &k = h->knob;                       // (test knobs, in the kernels' arguments)
    d.trace_until = k.trace_until; d.cand_d = k.cand_d; d.cand_pairwise = k.cand_pairwise; d.cls_rows_max = k.cls_rows_max; d.win_offset = k.win_offset;
    d.cand_zoom = k.cand_zoom; d.cand_speculate = k.cand_speculate; d.cand_take_all = k.cand_take_all; d.poll_delay = k.poll_delay; d.cand_others = k.cand_others;
    int rc = alloc_weights(h);
    rc |= alloc_stream_state(h);
    if (rc) return fail_create(h, h->err, HTM_ERR_HIP);
    if (hipHostMalloc((void **)&h->seg_pinned, sizeof(int), hipHostMallocDefault) == hipSuccess) *h->seg_pinned = 0; else h->seg_pinned = nullptr;
    size_launches(h);
    e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail_create(h, std::string("hipStreamSynchronize: ") + hipGetErrorString(e), HTM_ERR_HIP);
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        g_registry.push_back(h);
    }
    refresh_exchange_mode(h);
    *out = h;
    return HTM_OK;
}

// ------------------------------------------------------------------------------------------
// Inference views (htm_create_view)

#define REFUSE_ON_VIEW(h, what)                                                                                   \
    do {                                                                                                          \
        if ((h)->is_view) {                                                                                       \
            (h)->err = std::string(what) + ": not available on an inference view (it shares its parent's weights and never learns)"; \
            return HTM_ERR_STATE;                                                                                 \
        }                                                                                                         \
    } while (0)

// a parent call that may change the weights: the views' per-cell maxima were made against rows that may since have moved to
// other cells, and their next learning role clears all of them (cm_dense_step, as after a state import)
static void weights_touched(htm_handle *h) {
    if (h->shared && !h->is_view) {
        std::lock_guard<std::mutex> lock(g_shared_mutex);
        h->shared->wgen += 1;
    }
}

// The start of every stepping call on a view (and a no-op on any other handle): the parent's held-back launch goes first, a parent
// that is ahead refuses the call, and the parent's segment count comes over on the shared stream (not a captured node: this runs
// before any capture).  learning != 0 is refused.
static int view_enter(htm_handle *h, int learning) {
    if (!h->is_view) return 0;
    if (learning) { h->err = "an inference view steps with learning = 0 only (it shares its parent's weights)"; return HTM_ERR_STATE; }
    htm_handle *par;
    long long wgen;
    {
        std::lock_guard<std::mutex> lock(g_shared_mutex);
        par = h->shared->parent;
        wgen = h->shared->wgen;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (par) {
        flush_tail(par);
        if (sp_is_ahead(par)) {
            h->err = "the view's parent is ahead (its htm_run ended with HTM_RUN_CONTINUE): finish the parent's run first";
            return HTM_ERR_STATE;
        }
        HIPCHK(h, hipMemcpyAsync(&h->d.ctr->S, &par->d.ctr->S, sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
        refresh_seg_hint(par);
        h->seg_hint = std::max(h->seg_hint, par->seg_hint);
    }
    if (wgen != h->seen_wgen) {
        h->seen_wgen = wgen;
        h->dense_step = (uint32_t)h->step_host + 1u;
        HIPCHK(h, hipMemcpyAsync(&h->d.ctr->cm_dense_step, &h->dense_step, sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));     // (the source is a host word the next call rewrites)
    }
    return 0;
}

extern "C" int htm_create_view(htm_handle *parent, htm_handle **out) {
    if (!out) return fail_create(nullptr, "htm_create_view: null argument", HTM_ERR_ARGUMENT);
    *out = nullptr;
    if (!parent) return fail_create(nullptr, "htm_create_view: null parent", HTM_ERR_ARGUMENT);
    if (parent->is_view) return fail_create(nullptr, "htm_create_view: the parent is a view itself (make views of the model that owns the weights)", HTM_ERR_STATE);
    if (!parent->cfg.enable_sp || !parent->cfg.enable_tm) return fail_create(nullptr, "htm_create_view: the parent needs a Spatial Pooler and a Temporal Memory", HTM_ERR_STATE);
    if (parent->world > 1) return fail_create(nullptr, "htm_create_view: the parent is column-sharded", HTM_ERR_STATE);
    if (parent->cfg.cell_dim > 64) return fail_create(nullptr, "htm_create_view: cell_dim above 64", HTM_ERR_STATE);
    if (parent->phase_open || parent->shard_open) return fail_create(nullptr, "htm_create_view: the parent has a step open (htm_sp_phase)", HTM_ERR_STATE);
    if (hipSetDevice(parent->device) != hipSuccess) return fail_create(nullptr, "htm_create_view: hipSetDevice failed", HTM_ERR_HIP);
    flush_tail(parent);
    if (sp_is_ahead(parent)) return fail_create(nullptr, "htm_create_view: the parent is ahead (htm_run ended with HTM_RUN_CONTINUE)", HTM_ERR_STATE);
    {   // the parent's weights become shared (once): they, and the parent's own stream, now live as long as the last view
        std::lock_guard<std::mutex> lock(g_shared_mutex);
        if (!parent->shared) {
            HtmShared *sh = new HtmShared();
            sh->allocs.swap(parent->weight_allocs);
            sh->stream = parent->stream;
            sh->own_stream = parent->own_stream;
            sh->parent = parent;
            sh->refs = 1;
            sh->wgen = 0;
            parent->own_stream = false;
            parent->shared = sh;
        }
    }
    // a fresh handle with the parent's shape, weights, knobs and launch sizes and where its stream is (step, segment count, select
    // window); its own stream state -- and none of the parent's buffers, graphs, events or descriptors
    htm_handle *h = new htm_handle();
    h->cfg = parent->cfg;
    h->device = parent->device;
    h->stream = parent->stream;
    h->rank = parent->rank;
    h->world = parent->world;
    h->d = parent->d;                                // (alloc_stream_state replaces the stream state's buffers)
    h->d.trace = nullptr;
    h->knob = parent->knob;
    h->sz = parent->sz;
    h->step_host = parent->step_host;
    h->seg_hint = parent->seg_hint;
    h->window_known = parent->window_known;
    h->is_view = true;
    h->knob.defer_tail = 0;                          // (a view's step is whole when its call returns: see view_enter)
    {   // (the shared scan's knobs are the view's own, read now: a group's form follows its first member's; and its own trace)
        const Knobs now = read_knobs();
        h->knob.shared_scan = now.shared_scan;
        h->knob.shared_members = now.shared_members;
        h->knob.trace = now.trace;
    }
    {
        std::lock_guard<std::mutex> lock(g_shared_mutex);
        h->shared = parent->shared;
        h->shared->refs += 1;
        h->seen_wgen = h->shared->wgen;
    }
    Dev &d = h->d;
    const Dev &pd = parent->d;
    int rc = alloc_stream_state(h);
    if (rc) return fail_create(h, h->err, HTM_ERR_HIP);
    // the parent's duty cycles and counter block, then a sequence reset (htm_reset.h) -- and the learning role's counts and the
    // sticky capacity flags start clean
    bool ok = hipMemcpyAsync(d.duty, pd.duty, (size_t)d.C * sizeof(float), hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
              hipMemcpyAsync(d.ctr, pd.ctr, sizeof(Counters), hipMemcpyDeviceToDevice, h->stream) == hipSuccess &&
              hipMemsetAsync(d.ctr->n_work, 0, sizeof(d.ctr->n_work), h->stream) == hipSuccess &&
              hipMemsetAsync(d.ctr->n_bind, 0, sizeof(d.ctr->n_bind), h->stream) == hipSuccess &&
              hipMemsetAsync(&d.ctr->error, 0, sizeof(int32_t), h->stream) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_tm_reset, dim3(reset_blocks(d)), dim3(256), 0, h->stream, d, (int)(h->step_host & 1), (const ResetDev *)nullptr,
                           (RecDev *)nullptr, (uint32_t)h->step_host);
        ok = hipGetLastError() == hipSuccess;
    }
    if (hipHostMalloc((void **)&h->seg_pinned, sizeof(int), hipHostMallocDefault) == hipSuccess) *h->seg_pinned = parent->seg_hint; else h->seg_pinned = nullptr;
    if (!ok || hipStreamSynchronize(h->stream) != hipSuccess) return fail_create(h, "htm_create_view: copying the parent's stream state failed", HTM_ERR_HIP);
    {
        std::lock_guard<std::mutex> lock(g_registry_mutex);
        g_registry.push_back(h);
    }
    refresh_exchange_mode(h);
    *out = h;
    return HTM_OK;
}

extern "C" int64_t htm_device_bytes(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    return h->own_bytes;
}

// ------------------------------------------------------------------------------------------
// Stream forks (htm_fork.h)

// The buffers of alloc_stream_state that are stream state, as k_stream_fork's table (a handle with SP and TM, unsharded: what
// views are made of).  Not in it: input_stage and d_cols_stage (a host-fed step writes them before it reads them), work,
// recyc_cnt, recyc_cnt2, recyc_need and dead_list (the learning role's: a view never learns, and its counts start clean), trace.
static ForkTable fork_table(const Dev &v, const Dev &s) {
    ForkTable t;
    memset(&t, 0, sizeof(t));
    int blocks = 0;
    auto add = [&](void *dst, const void *src, size_t bytes, int kind) {
        ForkEntry &e = t.e[t.n++];
        e.dst = (unsigned char *)dst;
        e.src = (const unsigned char *)src;
        e.bytes = bytes;
        e.kind = kind;
        e.first_block = blocks;
        e.blocks = fork_blocks(bytes);
        blocks += e.blocks;
    };
    const size_t C = v.C, k = v.k, KP = v.KP, WPC = v.WPC, S = v.Lcap;
    const size_t colwords_padded = (size_t)((C + 255) / 256) * 8;
    // the largest first: their blocks start first
    for (int q = 0; q < 2; ++q) add(v.cellmax[q], s.cellmax[q], C * KP * 4, FORK_FIXED);
    add(v.seg_info, s.seg_info, S * 4, FORK_ROWS);
    add(v.seg_jit, s.seg_jit, S * 4, FORK_ROWS);
    for (int q = 0; q < 2; ++q) add(v.match_bits[q], s.match_bits[q], (S + 255) / 256 * 8 * 4, FORK_BITS);
    for (int q = 0; q < 2; ++q) {
        add(v.boosted[q], s.boosted[q], C * 8, FORK_FIXED);
        add(v.key[q], s.key[q], C * 8, FORK_FIXED);
        add(v.overlap[q], s.overlap[q], C * 4, FORK_FIXED);
        add(v.act[q], s.act[q], C * WPC * 4, FORK_FIXED);
        add(v.pred[q], s.pred[q], C * WPC * 4, FORK_FIXED);
        add(v.win[q], s.win[q], C * WPC * 4, FORK_FIXED);
        add(v.winners[q], s.winners[q], k * KP * 4, FORK_FIXED);
        add(v.active_cols[q], s.active_cols[q], (k + 8) * 4, FORK_FIXED);
        add(v.colbits[q], s.colbits[q], colwords_padded * 4, FORK_FIXED);
        add(v.col_rank[q], s.col_rank[q], colwords_padded * 2, FORK_FIXED);
    }
    add(v.duty, s.duty, C * 4, FORK_FIXED);
    add(v.hist, s.hist, (size_t)2 * SEL_MAX_PASSES * SEL_BINS * 4, FORK_FIXED);
    add(v.hist0, s.hist0, (size_t)2 * HIST0_PAR * 4, FORK_FIXED);
    add(v.sel_blk, s.sel_blk, (C + 255) / 256 * 4, FORK_FIXED);
    add(v.sel_rec, s.sel_rec, (C + 255) / 256 * 32 * 4, FORK_FIXED);
    add(v.fan, s.fan, (size_t)2 * FAN_COUNTERS * FAN_STRIDE * 4, FORK_FIXED);
    add(v.bursting, s.bursting, k, FORK_FIXED);
    add(v.actw_id, s.actw_id, (k * WPC + 8) * 4, FORK_FIXED);
    add(v.winw_idx, s.winw_idx, (k * WPC + 8) * 4, FORK_FIXED);
    add(v.actcnt, s.actcnt, k * WPC + 8, FORK_FIXED);
    add(v.act_list, s.act_list, (k * WPC + 16) * 4, FORK_FIXED);
    add(v.unacc_word, s.unacc_word, (k * WPC + 8) * 4, FORK_FIXED);
    add(v.unacc_list, s.unacc_list, k * KP * 4, FORK_FIXED);
    static_assert(2 + 2 + 2 + 2 * 10 + 13 <= FORK_MAX_ENTRIES, "k_stream_fork's table holds every entry");
    return t;
}

// After the source's (and the parent's) held-back launch: one launch on the shared stream, no copy, no wait.  The view then IS the
// source as far as a step with learning = 0 can tell, the host's part of the stream included -- and its per-cell maxima are the
// source's, as current with the weights as the source's own: the view takes the source's generation of the weights and its
// cm_dense_step, so that the next view_enter has nothing to say and does not wait (a look-ahead syncs before every window).
extern "C" int htm_view_sync(htm_handle *view, htm_handle *source) {
    if (!view || !source) return HTM_ERR_ARGUMENT;
    if (view == source) { view->err = "htm_view_sync: the view and the source are one handle"; return HTM_ERR_STATE; }
    if (!view->is_view) { view->err = "htm_view_sync: the first handle is not an inference view (htm_create_view)"; return HTM_ERR_STATE; }
    if (!source->shared || source->shared != view->shared) {
        view->err = "htm_view_sync: the source is neither the view's parent nor another view of it (the handles do not share weights)";
        return HTM_ERR_STATE;
    }
    if (view->phase_open || view->shard_open || source->phase_open || source->shard_open) {
        view->err = "htm_view_sync: a step of the view or of the source is open (htm_sp_phase)";
        return HTM_ERR_STATE;
    }
    htm_handle *par;
    long long wgen;
    {
        std::lock_guard<std::mutex> lock(g_shared_mutex);
        par = view->shared->parent;
        wgen = view->shared->wgen;
    }
    if (sp_is_ahead(view) || sp_is_ahead(source) || (par && sp_is_ahead(par))) {
        view->err = "htm_view_sync: the view, the source or the parent is ahead (its htm_run ended with HTM_RUN_CONTINUE): finish that run first";
        return HTM_ERR_STATE;
    }
    HIPCHK(view, hipSetDevice(view->device));
    flush_tail(source);
    if (par && par != source) flush_tail(par);
    // (the parent is gone: nobody hands this view a segment count again, and an earlier run of the view may still be copying
    // its own into the pinned word)
    if (!par) HIPCHK(view, hipStreamSynchronize(view->stream));
    const ForkTable t = fork_table(view->d, source->d);
    const ForkEntry &last = t.e[t.n - 1];
    LAUNCH(view, "stream_fork", k_stream_fork, last.first_block + last.blocks, FORK_THREADS, t, view->d.ctr, (const Counters *)source->d.ctr);
    const int rc = launch_status(view->err);
    if (rc) return rc;
    // (the pinned word below is written from the host while a copy an earlier run of the view queued into it may still be in
    // flight.  With a live parent that needs no wait: whichever lands last, the word holds a segment count the shared store has
    // reached, refresh_seg_hint only ever takes the larger of it and the hint, and the view's next call takes the parent's
    // count in view_enter before anything reads the bound.  Only a view whose parent is gone keeps what it is given here: that
    // case waited above.)
    refresh_seg_hint(source);
    view->step_host = source->step_host;
    view->seg_hint = source->seg_hint;
    if (view->seg_pinned) *view->seg_pinned = source->seg_hint;
    view->window_known = source->window_known;
    view->seen_wgen = source->is_view ? source->seen_wgen : wgen;
    view->dense_step = source->dense_step;
    return HTM_OK;
}

// Rows of a device bank, contiguous: dst row r = bank row (first_step + r) % bank_rows -- the rows a run of n steps from step
// index first_step read, or (with feedback) wrote.  One launch on the handle's stream, no wait.
extern "C" int htm_bank_rows(htm_handle *h, const uint32_t *device_bank, int32_t bank_rows, int64_t first_step, int32_t n, uint32_t *device_dst) {
    if (!h || !device_bank || !device_dst) return HTM_ERR_ARGUMENT;
    if (bank_rows < 1 || first_step < 0 || n < 0 || n > bank_rows) { h->err = "htm_bank_rows: bank_rows >= 1, first_step >= 0 and 0 <= n <= bank_rows"; return HTM_ERR_ARGUMENT; }
    if ((((uintptr_t)device_bank | (uintptr_t)device_dst) & 15) != 0) { h->err = "htm_bank_rows: the bank and the destination must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    if (!h->cfg.enable_sp) { h->err = "htm_bank_rows: needs a handle with the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
    if (n == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    LAUNCH(h, "bank_rows", k_bank_rows, n, 256, device_bank, (int)bank_rows, (int)(first_step % bank_rows), h->d.W4, device_dst);
    return launch_status(h->err);
}

// TemporalMemory.process(..., epsilon=) (networks.py:91): the tolerance of the "best matching" / "least used" ties
// (networks.py:81,88; projections.py:267), compared as float32.  0 < epsilon <= 1: the other uses (prediction > epsilon,
// potential < epsilon) then mean what they mean at 1e-8.  Kernels get it with their arguments: cached graphs are dropped.
extern "C" int htm_set_epsilon(htm_handle *h, float epsilon) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    if (!(epsilon > 0.f) || epsilon > 1.f) { h->err = "htm_set_epsilon: need 0 < epsilon <= 1"; return HTM_ERR_ARGUMENT; }
    REJECT_WHEN_AHEAD(h);
    if (epsilon == h->d.eps) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (auto &kv : h->graphs) hipGraphExecDestroy(kv.second);
    h->graphs.clear();
    h->d.eps = epsilon;
    return HTM_OK;
}

extern "C" int htm_get_stream(htm_handle *h, void **stream) {
    if (!h || !stream) return HTM_ERR_ARGUMENT;
    *stream = (void *)h->stream;
    return HTM_OK;
}

extern "C" int htm_sync(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    HIPCHK(h, hipSetDevice(h->device));
    // a short run ends within a millisecond: poll for that long (a blocking wait is woken tens of microseconds late),
    // then block
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(h->stream);
        if (e == hipSuccess) return HTM_OK;
        if (e != hipErrorNotReady) { h->err = std::string("hipStreamQuery: ") + hipGetErrorString(e); return HTM_ERR_HIP; }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

static int check_rows(htm_handle *h, const void *rows, int row_begin, int row_count) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!h->cfg.enable_sp) { h->err = "handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    if (!rows || row_begin < 0 || row_count < 0 || row_begin + (long long)row_count > h->d.C) {
        h->err = "permanence rows out of range";
        return HTM_ERR_ARGUMENT;
    }
    return 0;
}

extern "C" int htm_sp_set_permanence(htm_handle *h, const double *rows, int32_t row_begin, int32_t row_count) {
    if (h) REFUSE_ON_VIEW(h, "htm_sp_set_permanence");
    if (h) flush_tail(h);
    if (h) weights_touched(h);
    int rc = check_rows(h, rows, row_begin, row_count);
    if (rc) return rc;
    REJECT_WHEN_AHEAD(h);
    if (row_count == 0) return HTM_OK;
    Dev &d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(d.perm + (size_t)row_begin * d.Ipad, (size_t)d.Ipad * 8, rows, (size_t)d.I * 8,
                               (size_t)d.I * 8, (size_t)row_count, hipMemcpyHostToDevice, h->stream));
    const long long waves = (long long)row_count * (d.Ipad / 64);
    const int blocks = (int)std::min<long long>((waves + 3) / 4, 8192);
    hipLaunchKernelGGL(k_sp_build_mask, dim3(blocks), dim3(256), 0, h->stream, d, row_begin, row_count);
    if (d.planes) hipLaunchKernelGGL(k_sp_build_planes, dim3((row_count + 63) / 64, (4 * d.W + 63) / 64), dim3(256), 0, h->stream, d, row_begin, row_count);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

extern "C" int htm_sp_get_permanence(htm_handle *h, double *rows, int32_t row_begin, int32_t row_count) {
    if (h) flush_tail(h);
    int rc = check_rows(h, rows, row_begin, row_count);
    if (rc) return rc;
    REJECT_WHEN_AHEAD(h);
    if (row_count == 0) return HTM_OK;
    Dev &d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(rows, (size_t)d.I * 8, d.perm + (size_t)row_begin * d.Ipad, (size_t)d.Ipad * 8,
                               (size_t)d.I * 8, (size_t)row_count, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

// The byte planes of the connected mask against the mask itself, compared on the device, and how many steps counted their
// overlap from the planes.
extern "C" int htm_sp_planes_check(htm_handle *h, int64_t out[2]) {
    if (!h || !out) return HTM_ERR_ARGUMENT;
    flush_tail(h);
    if (!h->cfg.enable_sp) { h->err = "handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    Dev &d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t steps = 0;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(&steps, &d.ctr->plane_steps, sizeof(steps), hipMemcpyDeviceToHost));
    out[0] = -1;
    out[1] = (int64_t)steps;
    if (!d.planes) return HTM_OK;
    if (!h->d_planes_bad) { if (int rc = dalloc(h, &h->d_planes_bad, 1)) return rc; }
    HIPCHK(h, hipMemsetAsync(h->d_planes_bad, 0, sizeof(unsigned long long), h->stream));
    const size_t total = (size_t)4 * d.W * d.plane_stride;
    hipLaunchKernelGGL(k_sp_planes_check, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, h->stream, d, h->d_planes_bad);
    unsigned long long bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, h->d_planes_bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    out[0] = (int64_t)bad;
    return HTM_OK;
}

// htm_sp_phase leaves the current (not yet closed) timestep half done: keys, boosted overlaps and the top-digit
// histogram of parity step_host & 1 (DenseProjection.process / ExponentialBoosting.process called on their own on the
// objects of a live SpatialPooler).  An entry point that runs the WHOLE step starts over: the histogram its overlap
// accumulates into must be clean (only a select clears it), and the Spatial Pooler fields htm_read returns are the last
// completed step's again.
static int close_open_phases(htm_handle *h) {
    if (!h->phase_open) return 0;
    const int p = (int)(h->step_host & 1);
    if (h->cfg.enable_sp) HIPCHK(h, clear_front_hist(h, p));
    h->phase_open = false;
    h->phase_active = 0;
    h->phase_wide = false;
    return 0;
}

static int stage_input(htm_handle *h, const uint32_t *packed_input) {
    Dev &d = h->d;
    const int words = (d.I + 31) / 32;
    HIPCHK(h, hipMemcpyAsync(d.input_stage, packed_input, (size_t)words * 4, hipMemcpyHostToDevice, h->stream));
    return 0;
}

static decltype(&k_learn_scan_front<1>) const kt_learn_scan_front[4] = {k_learn_scan_front<1>, k_learn_scan_front<2>, k_learn_scan_front<4>, k_learn_scan_front<8>};

// One host-fed step (htm_step: one input per call; an input too wide for a launch's arguments is already staged).
// Three launches per step for a caller that steps and steps: the learning role and the scan of a step need nothing of the
// NEXT input and nothing the next step's overlap touches -- they are held back and ride beside that overlap (the
// permanence rows, which the overlap does read, in the middle launch instead).  Any other call lets them go first.
static int enqueue_hostfed(htm_handle *h, const uint32_t *packed_input, int learning) {
    Dev &d = h->d;
    if (!(h->knob.defer_tail && d.W <= ARG_INPUT_WORDS && tm_tail_fused(h) && !h->profile)) {
        flush_tail(h);
        return enqueue_step(h, RunModes{}, d.input_stage, 1, learning, StepPlan{false, false, false}, packed_input);
    }
    const int p = (int)(h->step_host & 1), wmode = step_wmode(h);
    // the held-back learning role and scan of the step before ride beside THIS step's select finish (k_learn_scan_emit, the last
    // launch of htm_run's schedules) where that launch is available: the overlap then has the first launch to itself (4.5 us), and the
    // select finish -- 7 us of a chain on 256 blocks -- no longer has the GPU to itself.  (The activation, which reads the
    // predictions that scan leaves, has moved behind it: k_act_mid_rows.)
    const bool ride_emit = h->knob.step_split && h->tail_pending && wmode && h->emit_fused && can_lean(h);
    if (ride_emit) {
        enqueue_sp_front(h, d.input_stage, 1, p, wmode, packed_input);
        h->tail_pending = false;
        launch_learn_scan_emit(h, h->tail_p, h->sz.c256_blocks);
        h->window_known = true;
    } else if (h->tail_pending) {                   // ... else beside this step's overlap (k_learn_scan_front)
        const LearnScan ls = learn_scan(h, (size_t)(SEL_BINS + ARG_INPUT_WORDS) * 4);
        h->tail_pending = false;
        LAUNCH_ON(h, h->stream, ls.lds, "tm_learn+tm_scan+sp_overlap", kt_learn_scan_front[ls.slot], ls.blocks() + h->sz.lean_overlap_blocks, 256,
                  d, h->tail_p, ls.n_learn, ls.n_scan, ls.spec, packed_input_arg(d, packed_input), h->sz.G, p, wmode);
        if (!wmode) launch_sel_passes(h, d, p);
    } else {
        enqueue_sp_front(h, d.input_stage, 1, p, wmode, packed_input);
    }
    if (h->knob.step_split) {
        // the select finish on its own (winner list and column bitmap, nothing else), then the two-launch schedule's first launch
        // in the form its last step takes: activation -> fan-in -> middle role beside the winner rows, the duty cycle and the
        // clears (k_act_mid_rows without an overlap role).  The activation no longer waits at the end of the select finish's
        // blocks with nothing beside it, and the rows stream under the Temporal Memory's chain (measured: DESIGN.md section 4)
        if (!ride_emit) enqueue_sp_back(h, d.input_stage, 1, p, 1, 0, false, wmode);
        launch_act_mid_rows(h, "tm_activate+tm_mid+sp_learn", 0, p, learning, d.input_stage, 1, 0);
        h->tail_pending = true;
        h->tail_p = p;
    } else {
        enqueue_sp_back(h, d.input_stage, 1, p, 1, EMIT_ALL, false, wmode);
        enqueue_tm(h, d.k, learning, 1, p, d.input_stage, 1, true, -1, true);
    }
    h->step_host += 1;
    return launch_status(h->err);
}

extern "C" int htm_step(htm_handle *h, const uint32_t *packed_input, int32_t learning) {
    if (!h || !packed_input) return HTM_ERR_ARGUMENT;
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_sp || !h->cfg.enable_tm) { h->err = "htm_step needs a handle with SP and TM"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "sharded handle: use htm_shard_begin / htm_shard_finish"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = view_enter(h, learning);
    if (rc) return rc;
    if (learning) weights_touched(h);
    refresh_exchange_mode(h);
    rc = close_open_phases(h);
    if (rc) return rc;
    if (h->d.W > ARG_INPUT_WORDS) {                 // (an input too wide for the launch's arguments: staged by a copy)
        flush_tail(h);
        rc = stage_input(h, packed_input);
        if (rc) return rc;
    }
    return enqueue_hostfed(h, packed_input, learning ? 1 : 0);
}

extern "C" int htm_sp_step(htm_handle *h, const uint32_t *packed_input, int32_t learning) {
    if (!h || !packed_input) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_sp) { h->err = "handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    // a handle that also owns a Temporal Memory steps both layers together: an SP-only step would skip the SP
    // learning that rides in the TM's middle launch and leave the TM's parity buffers one step behind
    if (h->cfg.enable_tm) { h->err = "htm_sp_step: the handle also has a Temporal Memory; use htm_step"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    refresh_exchange_mode(h);
    int rc = close_open_phases(h);
    if (rc) return rc;
    rc = stage_input(h, packed_input);
    if (rc) return rc;
    const int p = (int)(h->step_host & 1);
    enqueue_sp_front(h, h->d.input_stage, 1, p, step_wmode(h));
    enqueue_sp_back(h, h->d.input_stage, 1, p, 0, EMIT_ALL, learning && !h->cfg.enable_tm, step_wmode(h));
    h->step_host += 1;
    return HTM_OK;
}

// SpatialPooler.process (networks.py:26-35) one phase per call, for plug-in objects that live on the host: the caller
// (bithtm_amd/networks.py) interleaves these with the `process` / `update` methods of the user's objects.
extern "C" int htm_sp_phase(htm_handle *h, int32_t phase, const void *data, int64_t count) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_sp) { h->err = "handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_sp_phase: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REFUSE_ON_VIEW(h, "htm_sp_phase");
    if (phase == HTM_SP_LEARN) weights_touched(h);
    HIPCHK(h, hipSetDevice(h->device));
    refresh_exchange_mode(h);
    Dev &d = h->d;
    const int p = (int)(h->step_host & 1);
    const int c256 = (d.C + 255) / 256;
    // values from the host are checked before anything is enqueued: a refused call leaves the handle as it was
    if (phase == HTM_SP_BOOST) {
        if (!data || count != d.C) { h->err = "htm_sp_phase(BOOST): need column_dim overlaps"; return HTM_ERR_ARGUMENT; }
        const int32_t *ov = (const int32_t *)data;
        for (int64_t i = 0; i < count; ++i)
            if (ov[i] < 0) { h->err = "htm_sp_phase(BOOST): overlaps are counts, column " + std::to_string(i) + " has a negative one"; return HTM_ERR_ARGUMENT; }
    }
    if (phase == HTM_SP_SELECT && data) {
        if (count != d.C) { h->err = "htm_sp_phase(SELECT): need column_dim boosted overlaps"; return HTM_ERR_ARGUMENT; }
        const double *bo = (const double *)data;
        for (int64_t i = 0; i < count; ++i)
            if (!(bo[i] >= 0.0) || bo[i] > DBL_MAX) {       // (NaN fails the first comparison; -0.0 passes: it is zero)
                h->err = "htm_sp_phase(SELECT): boosted overlaps must be finite and >= 0 (any double in [0, DBL_MAX], -0.0 counts as 0); column " +
                         std::to_string(i) + " is NaN, infinite or negative";
                return HTM_ERR_ARGUMENT;
            }
    }
    // Keys made from the host's values are selected at full width: the fused step's shortcuts -- low_zero key bits known to be
    // zero, the last digits left to role_emit's record exchange -- rest on boosted = float32 factor x overlap <= input_dim,
    // which a caller's own numbers need not obey.  All SEL_MAX_PASSES digits are launched on a copy of the descriptor (the
    // handle's own, which htm_step, htm_run and the graphs see, is untouched), then the count and the plain emit.
    Dev wide = d;
    wide.sel_passes = SEL_MAX_PASSES;
    wide.low_zero = 0;
    // the top-digit histogram of this step's keys is accumulated by the phase that makes the keys and consumed (and
    // cleared) by the select: a phase that makes keys starts from a clean one, whatever ran before it in this step
    if (phase == HTM_SP_OVERLAP || phase == HTM_SP_BOOST || (phase == HTM_SP_SELECT && data))
        HIPCHK(h, clear_front_hist(h, p));
    switch (phase) {
        case HTM_SP_OVERLAP: {                     // DenseProjection.process + ExponentialBoosting.process; data = packed input
            if (!data) return HTM_ERR_ARGUMENT;
            int rc = stage_input(h, (const uint32_t *)data);
            if (rc) return rc;
            LAUNCH(h, "sp_overlap", k_sp_overlap, h->sz.sp_blocks, RB, d, d.input_stage, 1, h->sz.G, p, p, 0, 0);
            h->phase_wide = false;
            break;
        }
        case HTM_SP_BOOST: {                       // ExponentialBoosting.process on overlaps from the host; data = int32[C]
            HIPCHK(h, hipMemcpyAsync(d.overlap[p], data, (size_t)d.C * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));         // (the caller's buffer is borrowed for the call only)
            LAUNCH(h, "sp_keys", k_sp_keys, std::min((d.C + RB - 1) / RB, 256), RB, wide, p, SP_KEYS_BOOST);
            h->phase_wide = true;
            break;
        }
        case HTM_SP_SELECT: {                      // GlobalInhibition.process; data = double[C] boosted overlaps, or NULL: the device's
            if (data) {
                HIPCHK(h, hipMemcpyAsync(d.boosted[p], data, (size_t)d.C * 8, hipMemcpyHostToDevice, h->stream));
                HIPCHK(h, hipStreamSynchronize(h->stream));
                LAUNCH(h, "sp_keys", k_sp_keys, std::min((d.C + RB - 1) / RB, 256), RB, wide, p, SP_KEYS_HOST);
                h->phase_wide = true;
            }
            if (h->phase_wide) {
                launch_sel_passes(h, wide, p);
                LAUNCH(h, "sp_count", k_sp_count, h->sz.c256_blocks, 256, wide, p);
                LAUNCH(h, "sp_emit", k_sp_emit, h->sz.c256_blocks, 256, wide, p, 0, 0, 0, 0, h->sz.c256_blocks);
                // (the k-th key of SP_KEYS_HOST is the double's own bits, not a select_key: it says nothing about where the fused
                // step's window should be -- the next whole step takes the digit passes, as a handle's first step does)
                h->window_known = !data;
            } else {
                launch_sel_passes(h, d, p);
                enqueue_sp_back(h, d.input_stage, 1, p, 0, 0, false);          // the list and its bitmap, nothing else
            }
            break;
        }
        case HTM_SP_ACTIVE: {                      // a winner list from the host; data = int32[count], distinct, any order
            if ((!data && count) || count < 0 || count > d.k) { h->err = "htm_sp_phase(ACTIVE): at most active_columns columns"; return HTM_ERR_ARGUMENT; }
            std::vector<int> cols((const int *)data, (const int *)data + count);
            std::sort(cols.begin(), cols.end());
            for (int64_t i = 0; i < count; ++i)
                if (cols[i] < 0 || cols[i] >= d.C || (i && cols[i] == cols[i - 1])) { h->err = "htm_sp_phase(ACTIVE): bad column list"; return HTM_ERR_ARGUMENT; }
            if (count) HIPCHK(h, hipMemcpyAsync(d.active_cols[p], cols.data(), (size_t)count * 4, hipMemcpyHostToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            h->phase_active = (int)count;
            h->phase_open = true;
            if (d.colbits[p]) {
                LAUNCH(h, "sp_list_bits", k_sp_list_bits, std::max(1, (d.colwords + 255) / 256), 256, d, p, (int)count, 0);
                if (count) LAUNCH(h, "sp_list_bits", k_sp_list_bits, (int)((count + 255) / 256), 256, d, p, (int)count, 1);
            }
            return HTM_OK;
        }
        case HTM_SP_LEARN:                         // DenseProjection.update on the current winner list, with the input of OVERLAP
            if (data) {
                int rc = stage_input(h, (const uint32_t *)data);
                if (rc) return rc;
            }
            if (h->phase_active) LAUNCH(h, "sp_learn", k_sp_learn, h->phase_active, 256, d, d.input_stage, 1, p);
            break;
        case HTM_SP_DUTY:                          // ExponentialBoosting.update on the current winner list
            LAUNCH(h, "sp_duty", k_sp_duty_list, c256, 256, d, p, h->phase_active, 0);
            if (h->phase_active) LAUNCH(h, "sp_duty", k_sp_duty_list, (h->phase_active + 255) / 256, 256, d, p, h->phase_active, 1);
            break;
        case HTM_SP_COMMIT:                        // close the step of a handle without Temporal Memory
            if (h->cfg.enable_tm) { h->err = "htm_sp_phase(COMMIT): the Temporal Memory's step closes the timestep (htm_tm_step)"; return HTM_ERR_STATE; }
            hipLaunchKernelGGL(k_sp_commit, dim3(1), dim3(1), 0, h->stream, d, p);
            h->step_host += 1;
            break;
        default: h->err = "htm_sp_phase: unknown phase"; return HTM_ERR_ARGUMENT;
    }
    if (phase == HTM_SP_SELECT) h->phase_active = d.k;
    h->phase_open = phase != HTM_SP_COMMIT;
    if (phase == HTM_SP_COMMIT) h->phase_wide = false;
    return launch_status(h->err);
}

extern "C" int htm_tm_step(htm_handle *h, const int32_t *active_column, int32_t n, int32_t learning, int32_t return_winner_cell) {
    if (!h || (!active_column && n > 0)) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_tm) { h->err = "handle has no Temporal Memory"; return HTM_ERR_STATE; }
    Dev &d = h->d;
    if (n < 0 || n > d.k) { h->err = "htm_tm_step: more active columns than active_columns"; return HTM_ERR_ARGUMENT; }
    {
        const int rc = view_enter(h, learning);
        if (rc) return rc;
        if (learning) weights_touched(h);
    }
    std::vector<int> cols(active_column, active_column + n);
    std::sort(cols.begin(), cols.end());
    for (int i = 0; i < n; ++i)
        if (cols[i] < 0 || cols[i] >= d.C || (i && cols[i] == cols[i - 1])) { h->err = "htm_tm_step: bad active column list"; return HTM_ERR_ARGUMENT; }
    HIPCHK(h, hipSetDevice(h->device));
    if (n) HIPCHK(h, hipMemcpyAsync(h->d_cols_stage, cols.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));      // cols is a local
    const int p = (int)(h->step_host & 1);
    const int want = (learning || return_winner_cell) ? 1 : 0;
    LAUNCH(h, "tm_load_active", k_tm_load_active, std::min((d.C + 255) / 256, 1024), 256, d, p, h->d_cols_stage, n);
    LAUNCH(h, "tm_activate", k_tm_activate, std::max(1, (n * d.KP + 255) / 256), 256, d, p, n, want);
    enqueue_tm(h, n, learning ? 1 : 0, want, p, nullptr, 1, false);
    h->step_host += 1;
    h->phase_open = false;
    return HTM_OK;
}

// PredictiveProjection.update (projections.py:257-293) called on its own: learning with the learning cells, the
// punishment mask and the previous State chosen by the caller.  The previous step's side -- prev_state, input_activation,
// winner_input -- is what the handle holds as its previous step (written there with the state import if it is not the
// handle's own: HTM_IMPORT_PREV_STATE).  columns[i] (distinct, any order, at most active_columns) has learning cells
// winner_words[i] (bit j = cell j; `output_learning` of :261-262 for that column; bits beyond the column's cells are ignored)
// of which unaccounted_words[i] need a new segment (:271: learning_output cells whose max jittered potential is below
// epsilon); punish_words: one word per column of the model, bit j = cell j of `output_punishment` (:269) -- any cells, learning
// cells included --, or NULL for "every cell of a column not listed" (what TemporalMemory passes, networks.py:107-108,111).
// Accepted beyond what the fused step forms: several learning cells per column up to all of them, punished learning cells,
// previous winners that are no subset of the previous activation.  Refused with HTM_ERR_ARGUMENT before anything is
// enqueued (the handle stays as it was): n above active_columns, a column listed twice or outside [0, column_dim), 65 536
// learning cells or more in one call (the middle launch packs its two running counts into 16 bits each).
// Order on one row: the learning update and its growth, then the punishment (:284-293) -- the punished rows are listed first
// (against the owners they have before any segment is recycled, :264), the middle launch classifies the learning rows only,
// and the punishment is a second learning launch behind the first (k_tm_ext_punish).
// Does not close the timestep: htm_tm_scan does.
extern "C" int htm_tm_update(htm_handle *h, const int32_t *columns, const uint32_t *winner_words, const uint32_t *unaccounted_words,
                             int32_t n, const uint32_t *punish_words) {
    if (!h || (n > 0 && (!columns || !winner_words || !unaccounted_words))) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_tm) { h->err = "handle has no Temporal Memory"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_tm_update: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REFUSE_ON_VIEW(h, "htm_tm_update");
    Dev &d = h->d;
    if (n < 0 || n > d.k) { h->err = "htm_tm_update: more columns with learning cells than active_columns"; return HTM_ERR_ARGUMENT; }
    // ascending columns (the order of the winner list, networks.py:103-104 under the ascending-column policy)
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return columns[a] < columns[b]; });
    std::vector<int> cols((size_t)n);
    const int WPC = d.WPC;                          // (the words: WPC per listed column)
    auto cells_of_word = [&](int hw) { const int cells = d.K - 32 * hw; return cells >= 32 ? 0xFFFFFFFFu : cells <= 0 ? 0u : ((1u << cells) - 1u); };
    std::vector<uint32_t> ww((size_t)n * WPC), uw((size_t)n * WPC);
    long long learning_cells = 0;
    for (int i = 0; i < n; ++i) {
        const int o = order[(size_t)i];
        cols[(size_t)i] = columns[o];
        for (int hw = 0; hw < WPC; ++hw) {
            const uint32_t w = winner_words[(size_t)o * WPC + hw] & cells_of_word(hw);
            ww[(size_t)i * WPC + hw] = w;
            uw[(size_t)i * WPC + hw] = unaccounted_words[(size_t)o * WPC + hw] & w;
            learning_cells += __builtin_popcount(w);
        }
        if (cols[(size_t)i] < 0 || cols[(size_t)i] >= d.C || (i && cols[(size_t)i] == cols[(size_t)i - 1])) {
            h->err = "htm_tm_update: bad column list (a column listed twice, or outside [0, column_dim))";
            return HTM_ERR_ARGUMENT;
        }
    }
    if (learning_cells >= 65536) {
        h->err = "htm_tm_update: " + std::to_string(learning_cells) + " learning cells in one call, at most 65535";
        return HTM_ERR_ARGUMENT;
    }
    weights_touched(h);
    HIPCHK(h, hipSetDevice(h->device));
    const int p = (int)(h->step_host & 1);
    int *d_cols = nullptr, *d_pcount = nullptr;
    uint32_t *d_ww = nullptr, *d_uw = nullptr, *d_pun = nullptr, *d_nopun = nullptr, *d_plist = nullptr;
    auto release = [&]() {
        for (void *ptr : {(void *)d_cols, (void *)d_ww, (void *)d_uw, (void *)d_pun, (void *)d_nopun, (void *)d_plist, (void *)d_pcount})
            if (ptr) hipFree(ptr);
    };
    const size_t nb = (size_t)std::max(n, 1) * 4, nbw = nb * WPC, pun_bytes = (size_t)d.C * WPC * 4;
    // punish_words == NULL: every cell of a column that is not listed (networks.py:107-108,111).  The mask is built here: the
    // middle launch's own default reads the step's active words, which this entry point does not write (htm_tm_scan does, later)
    std::vector<uint32_t> default_pun;
    if (!punish_words) {
        default_pun.resize((size_t)d.C * WPC);
        for (size_t w = 0; w < default_pun.size(); ++w) default_pun[w] = cells_of_word((int)(w % WPC));
        for (int i = 0; i < n; ++i)
            for (int hw = 0; hw < WPC; ++hw) default_pun[(size_t)cols[(size_t)i] * WPC + hw] = 0u;
        punish_words = default_pun.data();
    }
    if (hipMalloc((void **)&d_cols, nb) != hipSuccess || hipMalloc((void **)&d_ww, nbw) != hipSuccess || hipMalloc((void **)&d_uw, nbw) != hipSuccess ||
        hipMalloc((void **)&d_pun, pun_bytes) != hipSuccess || hipMalloc((void **)&d_nopun, pun_bytes) != hipSuccess ||
        hipMalloc((void **)&d_plist, (size_t)std::max(d.work_cap, 1) * 4) != hipSuccess || hipMalloc((void **)&d_pcount, 4) != hipSuccess) {
        release(); h->err = "htm_tm_update: hipMalloc failed"; return HTM_ERR_HIP;
    }
    bool ok = true;
    if (n) ok = hipMemcpyAsync(d_cols, cols.data(), nb, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
                hipMemcpyAsync(d_ww, ww.data(), nbw, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
                hipMemcpyAsync(d_uw, uw.data(), nbw, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    if (ok) ok = hipMemcpyAsync(d_pun, punish_words, pun_bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
                 hipMemsetAsync(d_nopun, 0, pun_bytes, h->stream) == hipSuccess && hipMemsetAsync(d_pcount, 0, 4, h->stream) == hipSuccess &&
                 // (the step's work counts start at zero: the scan before left them so; a second update without a scan between did not)
                 hipMemsetAsync(&d.ctr->n_work[p], 0, sizeof(int), h->stream) == hipSuccess &&
                 hipMemsetAsync(&d.ctr->n_bind[p], 0, sizeof(int), h->stream) == hipSuccess;
    if (!ok) { release(); h->err = "htm_tm_update: hipMemcpy failed"; return HTM_ERR_HIP; }
    static decltype(&k_tm_learn_ext<1>) const kt_tm_learn_ext[4] = {k_tm_learn_ext<1>, k_tm_learn_ext<2>, k_tm_learn_ext<4>, k_tm_learn_ext<8>};
    auto learn = [&]() { LAUNCH_ON(h, h->stream, learn_lds(learn_epl(d)), "tm_learn", kt_tm_learn_ext[epl_slot(d)], kLearnBlocks, RB, d, p); };
    const int pun_blocks = std::max(1, std::min((d.Scap + 255) / 256, 1024));
    hipLaunchKernelGGL(k_tm_ext_winners, dim3(std::min((d.C + 255) / 256, 1024)), dim3(256), 0, h->stream, d, p, d_cols, d_ww, d_uw, n, 0);
    if (n) hipLaunchKernelGGL(k_tm_ext_winners, dim3((n * WPC + 255) / 256), dim3(256), 0, h->stream, d, p, d_cols, d_ww, d_uw, n, 1);
    hipLaunchKernelGGL(k_tm_ext_punish, dim3(pun_blocks), dim3(256), 0, h->stream, d, p, d_pun, d_plist, d_pcount, 0);
    d.punish = d_nopun;                             // (kernels take Dev by value: set for the middle launch only -- it lists no punished row)
    LAUNCH(h, "tm_mid", k_mid_rows, 1 + kClassifyBlocks + h->sz.zero_blocks, 256, d, p, n, 1, 1, kClassifyBlocks, nullptr, 1, 0, 0, 0);
    d.punish = nullptr;
    learn();                                        // learn and grow ...
    hipLaunchKernelGGL(k_tm_ext_punish, dim3(pun_blocks), dim3(256), 0, h->stream, d, p, d_pun, d_plist, d_pcount, 1);
    learn();                                        // ... then punish
    hipError_t e = hipGetLastError();
    const bool synced = hipStreamSynchronize(h->stream) == hipSuccess;       // (the staging buffers are this call's)
    release();
    if (e != hipSuccess || !synced) { h->err = std::string("htm_tm_update: ") + hipGetErrorString(e != hipSuccess ? e : hipGetLastError()); return HTM_ERR_HIP; }
    h->phase_open = false;
    return HTM_OK;
}

// PredictiveProjection.process (projections.py:245-255) called on its own: the segment scan against the active cells the
// caller names (active_words: one word per column of the model, bit j = cell j), which become the step's cell activation;
// closes the timestep.  The State is read with htm_read (MATCH_*, SEG_POTENTIAL, CELL_MAX_JITTER, CELL_PREDICTION).
extern "C" int htm_tm_scan(htm_handle *h, const uint32_t *active_words) {
    if (!h || !active_words) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (!h->cfg.enable_tm) { h->err = "handle has no Temporal Memory"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_tm_scan: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    {
        const int rc = view_enter(h, 0);
        if (rc) return rc;
    }
    Dev &d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    const int p = (int)(h->step_host & 1);
    uint32_t *d_act = nullptr;
    if (hipMalloc((void **)&d_act, (size_t)d.C * d.WPC * 4) != hipSuccess) { h->err = "htm_tm_scan: hipMalloc failed"; return HTM_ERR_HIP; }
    bool ok = hipMemcpyAsync(d_act, active_words, (size_t)d.C * d.WPC * 4, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    // clean accumulators: the scan sets match bits, per-cell maxima and prediction bits with atomics (in a whole timestep the
    // middle launch and the learning role of the step before leave them clean)
    ok = ok && hipMemsetAsync(d.match_bits[p], 0, (size_t)(d.Lcap + 255) / 256 * 8 * 4, h->stream) == hipSuccess &&
         hipMemsetAsync(d.cellmax[p], 0, (size_t)d.C * d.KP * 4, h->stream) == hipSuccess &&
         hipMemsetAsync(&d.ctr->n_active_cells, 0, sizeof(int), h->stream) == hipSuccess;
    if (!ok) { hipFree(d_act); h->err = "htm_tm_scan: staging failed"; return HTM_ERR_HIP; }
    hipLaunchKernelGGL(k_tm_ext_active, dim3(std::min((d.C + 255) / 256, 1024)), dim3(256), 0, h->stream, d, p, d_act);
    launch_scan(h, p, bitmap_fits_lds(d));
    hipError_t e = hipGetLastError();
    const bool synced = hipStreamSynchronize(h->stream) == hipSuccess;
    hipFree(d_act);
    if (e != hipSuccess || !synced) { h->err = std::string("htm_tm_scan: ") + hipGetErrorString(e != hipSuccess ? e : hipGetLastError()); return HTM_ERR_HIP; }
    h->step_host += 1;
    h->phase_open = false;
    return HTM_OK;
}

// Whether a batched call of n_steps with these flags (HTM_RUN_*) replays graphs and (htm_run alone) runs pipelined on this handle now
// (a short call is launched eagerly whatever the flag says: a graph launch on an idle device starts its first kernel
// about 7 us later than a kernel launch does, and the host submits three launches per 30-us step with time to spare --
// measured, 20 steps per call: 615 against 638 us; from 64 steps on the graphs are level and then ahead)
struct RunSchedule { bool graph, pipeline; };
static RunSchedule run_schedule(const htm_handle *h, int n_steps, int flags) {
    return {(flags & 1) && !h->profile && n_steps >= h->knob.eager_below, !(flags & 2) && can_pipeline(h) && !decode_unpipelined(h) && !h->feed_bank};
}

// what every recorded call refuses about an htm_run_record (who: the call, or the group's member, the message names)
static int check_run_record(const htm_run_record &r, const std::string &who, std::string &err) {
    if (r.struct_bytes != sizeof(htm_run_record)) { err = who + ": struct_bytes != sizeof(htm_run_record)"; return HTM_ERR_ARGUMENT; }
    if (!r.records && !r.active_column && !r.column_prediction) { err = who + ": no record buffer given"; return HTM_ERR_ARGUMENT; }
    return 0;
}

// The setup of a batched call's modes (htm_run / htm_run_recorded, htm_tm_run): each mode's device descriptor, allocated on
// demand and -- unless the call only prepares graphs or has no steps (launch = false) -- filled by its begin launch.  n_bank: the
// rows of the call's bank; recorded: the call is a recorded one (rec: its buffers, checked by the caller; NULL when it only prepares).
static int begin_run_modes(htm_handle *h, int n_bank, int n_steps, bool recorded, const htm_run_record *rec, bool launch, RunModes *modes) {
    int rc;
    if (h->reset_bits) {
        if (!h->d_reset && (rc = dalloc(h, &h->d_reset, 1))) return rc;
        if (launch) LAUNCH(h, "tm_reset", k_reset_begin, 1, 64, h->d_reset, h->reset_bits, (int32_t)n_bank);
    }
    if (recorded) {
        if (!h->d_rec && (rc = dalloc(h, &h->d_rec, 1))) return rc;
        if (launch) {
            // the descriptor of this call, and the columns the last completed step predicts (predicted_columns_before of record 0)
            HIPCHK(h, hipMemsetAsync(h->d_rec, 0, sizeof(RecDev), h->stream));
            LAUNCH(h, "record", k_rec_begin, rec_blocks(h->d), 256, h->d, (int)((h->step_host + 1) & 1), h->d_rec, rec->records,
                   rec->active_column, rec->column_prediction, (uint32_t)h->step_host, n_steps);
        }
    }
    if (h->pin_out) {
        if (!h->d_pin && (rc = dalloc(h, &h->d_pin, 1))) return rc;
        if (launch) LAUNCH(h, "predicted_input", k_pin_begin, pin_begin_blocks(n_steps, h->d.I), 256, h->d_pin, h->pin_out, (uint32_t)h->step_host, n_steps, h->d.I);
    }
    *modes = RunModes{recorded, h->reset_bits != nullptr, h->pin_out != nullptr, h->feed_bank != nullptr, recorded && h->cap_out != nullptr};
    return 0;
}

// htm_run, or (dry) only the capture + instantiation of every hipGraph that call would replay; recorded (rec: NULL when dry) or not
struct RunCall { const uint32_t *bank; int32_t n_inputs, n_steps, learning, flags; bool dry; const htm_run_record *rec; bool recorded; };

static int run_or_prepare(htm_handle *h, const RunCall &c) {
    if (h) flush_tail(h);
    if (!h || !c.bank || c.n_inputs < 1 || c.n_steps < 0) return HTM_ERR_ARGUMENT;
    if (!h->cfg.enable_sp || !h->cfg.enable_tm) { h->err = "htm_run needs a handle with SP and TM"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "sharded handle: use htm_shard_begin / htm_shard_finish"; return HTM_ERR_STATE; }
    if (h->cap_out && !c.recorded) { h->err = "htm_run: active-cell rows are set (htm_set_run_active_cells): only a recorded run fills them"; return HTM_ERR_ARGUMENT; }
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = view_enter(h, c.learning)) return rc;
    const int n_inputs = c.n_inputs, learning = c.learning ? 1 : 0;
    int n_steps = c.n_steps;
    if (learning && !c.dry && n_steps > 0) weights_touched(h);
    refresh_exchange_mode(h);
    RunSchedule sched = run_schedule(h, n_steps, c.flags);
    bool resume = sp_is_ahead(h);                  // the previous call left the SP one step (and a front) ahead
    if (h->feed_bank) {                            // (htm_set_run_feedback: what a feeding call refuses)
        if (learning) { h->err = "htm_run: run feedback is set (htm_set_run_feedback): learning must be 0"; return HTM_ERR_ARGUMENT; }
        if (h->feed_bank != c.bank || h->feed_n != n_inputs) { h->err = "htm_run: run feedback was set for another bank or n_inputs (htm_set_run_feedback)"; return HTM_ERR_ARGUMENT; }
        if (h->reset_bits) { h->err = "htm_run: run feedback and reset bits are set at the same time (htm_set_run_feedback, htm_set_run_resets)"; return HTM_ERR_ARGUMENT; }
        if (resume) { h->err = "htm_run: run feedback is set while the Spatial Pooler is ahead (HTM_RUN_CONTINUE)"; return HTM_ERR_STATE; }
    }
    if (resume && (h->ahead_bank != c.bank || h->ahead_n_inputs != n_inputs || h->ahead_learning != learning)) {
        h->err = "htm_run: the previous call ended with HTM_RUN_CONTINUE; this one must use the same bank, n_inputs and learning flag";
        return HTM_ERR_STATE;
    }
    // keep looking ahead past the end of this call -- where the pipelined schedule is available (the flag is a promise of
    // the caller's, not a demand: without the schedule the call simply leaves nothing outstanding)
    const bool pipeline = sched.pipeline, cont = (c.flags & 4) && pipeline && n_steps > 0;
    if (h->reset_bits && h->reset_n != n_inputs) { h->err = "htm_run: the reset bits were set for a bank of another n_inputs (htm_set_run_resets)"; return HTM_ERR_ARGUMENT; }
    if (c.dry && !sched.graph) return HTM_OK;
    if (!c.dry) { int rc = close_open_phases(h); if (rc) return rc; }
    RunModes modes;
    if (int rc = begin_run_modes(h, n_inputs, n_steps, c.recorded, c.rec, !c.dry && n_steps > 0, &modes)) return rc;
    // The SP is ahead but the pipelined schedule is gone (another handle with its own stream has appeared on the device since,
    // or this call asks for HTM_RUN_NO_PIPELINE): the coming step is run as the LAST step of the run that went ahead -- its
    // launches hold no select finish, so nothing in them waits for another block -- and the rest of the call unpipelined.
    if (resume && !pipeline && n_steps > 0) {
        if (c.dry) return HTM_OK;                      // (that step is launched eagerly; the rest builds its graphs when it runs)
        const int p = (int)(h->step_host & 1);
        enqueue_run_reset(h, modes, p);
        (h->ahead_lean ? enqueue_lean : enqueue_pipelined)(h, p, learning, c.bank, n_inputs, StepPlan{true, false, false});
        enqueue_step_outputs(h, modes, p);
        h->step_host += 1;
        // (the four-launch schedule had begun the step after it: that front is never consumed)
        HIPCHK(h, clear_front_hist(h, (int)(h->step_host & 1)));
        h->ahead_bank = nullptr;
        if (int rc = launch_status(h->err)) return rc;
        n_steps -= 1;
        resume = false;
        sched = run_schedule(h, n_steps, c.flags);
    }
    // Graphs hold the launches of one step, or of up to kGraphSteps consecutive steady-state steps (a graph
    // launch boundary costs about 5 us more than a kernel boundary inside a graph: tools/step_timeline.py).
    // Nothing in a graph depends on the step index: kernels read it, and with it the bank row, from
    // the device counter.
    const int kGraphSteps = h->knob.graph_steps;
    refresh_seg_hint(h);                            // what the last run left
    bool sp_done = resume;                          // the SP has already done the coming step
    long long step = h->step_host;
    for (int t = 0; t < n_steps;) {
        const bool lean = pipeline && can_lean(h);      // (looks one step ahead, not two)
        const StepPlan plan{sp_done, pipeline && (t + 1 < n_steps || cont), pipeline && !lean && (t + 2 < n_steps || cont)};
        sp_done = plan.next_sp;
        if (!sched.graph) {
            int rc = enqueue_step(h, modes, c.bank, n_inputs, learning, plan);
            if (rc) return rc;
            t += 1;
            continue;
        }
        const int p = (int)(step & 1);
        // steady state: this and the next span - 1 steps all look ahead fully
        int span = 1;
        if (plan.sp_done && (lean ? plan.next_sp : plan.next_front)) {
            const int steady = cont ? n_steps - t : n_steps - t - (lean ? 1 : 2);       // steps from here on that look ahead fully
            if (cont && steady > 1 && steady < 2 * kGraphSteps) span = steady;      // a continuing call's (last) stretch: one graph
            else if (steady >= kGraphSteps) span = kGraphSteps;
        }
        if (!c.dry) {
            if (!plan.sp_done && !plan.next_sp) enqueue_sp_front(h, c.bank, n_inputs, p, step_wmode(h));    // eager
            enqueue_cold_start(h, c.bank, n_inputs, learning, plan);                         // eager: first step of a pipelined run
        }
        const RunGraphKey key{p, modes, learning, plan.sp_done, plan.next_sp, plan.next_front, lean,
                              scan_spec_blocks(h), scan_pool_is_large(h), h->emit_fused, step_wmode(h) != 0, span, c.bank, n_inputs};
        const hipGraphExec_t exec = cached_graph(h->graphs, key, h->stream, h->err, [&] {
            for (int i = 0; i < span; ++i) {
                enqueue_rest(h, modes, (p + i) & 1, c.bank, n_inputs, learning, plan);
                enqueue_step_outputs(h, modes, (p + i) & 1);
            }
            return 0;
        });
        if (!exec) return HTM_ERR_HIP;
        if (!c.dry) {
            HIPCHK(h, hipGraphLaunch(exec, h->stream));
            h->step_host += span;
        }
        step += span;
        t += span;
    }
    if (c.dry) return HTM_OK;
    if (n_steps > 0) {
        if (resume && !cont && n_steps == 1)        // the front computed for the step after this one is never consumed:
            HIPCHK(h, clear_front_hist(h, (int)(h->step_host & 1)));    // its digit histogram
        h->ahead_bank = cont ? c.bank : nullptr;
        h->ahead_lean = cont && can_lean(h);
        h->ahead_n_inputs = n_inputs;
        h->ahead_learning = learning;
        // leave the segment count where the next call finds it (no wait: it may see the one before)
        HIPCHK(h, hand_back_segments(h, &h->d.ctr->S, h->stream));
    }
    return HTM_OK;
}

extern "C" int htm_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning, int32_t use_graph) {
    return run_or_prepare(h, RunCall{device_inputs, n_inputs, n_steps, learning, use_graph, false, nullptr, false});
}

extern "C" int htm_prepare(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning, int32_t use_graph) {
    return run_or_prepare(h, RunCall{device_inputs, n_inputs, n_steps, learning, use_graph, true, nullptr, false});
}

// htm_run with a per-step record (include/bithtm_hip.h).  c.dry (htm_prepare_recorded): the graphs only -- they do not depend
// on the buffers, so there is no rec to check.
static int run_recorded(htm_handle *h, const RunCall &c) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h->world > 1) { h->err = "htm_run_recorded: a sharded handle has no recorded run"; return HTM_ERR_STATE; }
    // (k_rec_step sums its counts in 24-bit fields of one word: RecDev::acc)
    if (h->d.C >= (1 << 24)) { h->err = "htm_run_recorded: column_dim must be below 2^24"; return HTM_ERR_STATE; }
    if (!c.dry) { int rc = check_run_record(*c.rec, "htm_run_recorded", h->err); if (rc) return rc; }
    if (!h->d_rec) {                                // (ahead of whatever the call lets go first)
        HIPCHK(h, hipSetDevice(h->device));
        if (int rc = dalloc(h, &h->d_rec, 1)) return rc;
    }
    return run_or_prepare(h, c);
}

extern "C" int htm_run_recorded(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning,
                                int32_t use_graph, const htm_run_record *rec) {
    if (!rec) return htm_run(h, device_inputs, n_inputs, n_steps, learning, use_graph);
    return run_recorded(h, RunCall{device_inputs, n_inputs, n_steps, learning, use_graph, false, rec, true});
}

extern "C" int htm_prepare_recorded(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning,
                                    int32_t use_graph) {
    return run_recorded(h, RunCall{device_inputs, n_inputs, n_steps, learning, use_graph, true, nullptr, true});
}

// Batched stand-alone Temporal Memory run (include/bithtm_hip.h; htm_tm_feed.h): n_steps of htm_tm_step
// (return_winner_cell = 1) over a device bank of lists, without the host in the loop.  The launches of one step, in order.
static void enqueue_tm_run_step(htm_handle *h, RunModes m, int p, const int32_t *lists, int n_rows, int n, int learning) {
    Dev &d = h->d;
    enqueue_run_reset(h, m, p);
    LAUNCH_ON(h, h->stream, feed_lds(d), "tm_feed", k_tm_feed, std::min((d.C + 255) / 256, 1024), FEED_THREADS, d, p, lists, n_rows, n);
    LAUNCH(h, "tm_activate", k_tm_activate, std::max(1, (n * d.KP + 255) / 256), 256, d, p, n, 1);
    enqueue_tm(h, n, learning, 1, p, nullptr, 1, false);
    if (m.recording) LAUNCH(h, "record", k_tm_feed_record, rec_blocks(d), 256, d, p, h->d_rec, n);
}

extern "C" int htm_tm_run(htm_handle *h, const int32_t *device_lists, int32_t n_rows, int32_t n, int32_t n_steps, int32_t learning,
                          int32_t use_graph, const htm_run_record *rec) {
    if (!h) return HTM_ERR_ARGUMENT;
    flush_tail(h);
    if (!device_lists) { h->err = "htm_tm_run: null bank of lists"; return HTM_ERR_ARGUMENT; }
    Dev &d = h->d;
    if (n_rows < 1 || n < 1 || n > d.k || n > d.C || n_steps < 0) {
        h->err = "htm_tm_run: n_rows >= 1, 1 <= n <= active_columns and n_steps >= 0";
        return HTM_ERR_ARGUMENT;
    }
    if (rec) { int rc = check_run_record(*rec, "htm_tm_run", h->err); if (rc) return rc; }
    if (!h->cfg.enable_tm) { h->err = "htm_tm_run: the handle has no Temporal Memory"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_tm_run: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REFUSE_ON_VIEW(h, "htm_tm_run");
    REJECT_WHEN_AHEAD(h);
    if (h->shard_open || h->phase_open) { h->err = "htm_tm_run: a step of the handle is open (htm_shard_begin / htm_sp_phase)"; return HTM_ERR_STATE; }
    if (h->pin_out || h->feed_bank) { h->err = "htm_tm_run: decoding rows or run feedback are set (htm_set_run_predicted_input, htm_set_run_feedback)"; return HTM_ERR_STATE; }
    if (h->cap_out) { h->err = "htm_tm_run: active-cell rows are set (htm_set_run_active_cells): only a recorded htm_run fills them"; return HTM_ERR_STATE; }
    // (k_rec_step sums its counts in 24-bit fields of one word: RecDev::acc)
    if (rec && d.C >= (1 << 24)) { h->err = "htm_tm_run: a recorded run needs column_dim below 2^24"; return HTM_ERR_STATE; }
    if (feed_lds(d) > FEED_LDS_MAX) { h->err = "htm_tm_run: the column bitmap of this handle does not fit the LDS (column_dim above 524032)"; return HTM_ERR_ARGUMENT; }
    if (h->reset_bits && h->reset_n != n_rows) { h->err = "htm_tm_run: the reset bits were set for a bank of another n_rows (htm_set_run_resets)"; return HTM_ERR_ARGUMENT; }
    if (n_steps == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    learning = learning ? 1 : 0;
    if (learning) weights_touched(h);
    const bool graph = run_schedule(h, n_steps, use_graph).graph;
    RunModes modes;
    if (int rc = begin_run_modes(h, n_rows, n_steps, rec != nullptr, rec, true, &modes)) return rc;
    refresh_seg_hint(h);                            // what the last run left
    const int kGraphSteps = h->knob.graph_steps;
    for (int t = 0; t < n_steps;) {
        const int p = (int)(h->step_host & 1);
        if (!graph) {
            enqueue_tm_run_step(h, modes, p, device_lists, n_rows, n, learning);
            h->step_host += 1;
            t += 1;
            continue;
        }
        // (nothing in a graph depends on the step index: the feed launch reads it, and with it the bank row, from the counter block)
        const int span = n_steps - t >= kGraphSteps ? kGraphSteps : 1;
        const TmRunGraphKey key{p, modes, learning, scan_spec_blocks(h), scan_pool_is_large(h), span, device_lists, n_rows, n};
        const hipGraphExec_t exec = cached_graph(h->tm_graphs, key, h->stream, h->err, [&] {
            for (int i = 0; i < span; ++i) enqueue_tm_run_step(h, modes, (p + i) & 1, device_lists, n_rows, n, learning);
            return 0;
        });
        if (!exec) return HTM_ERR_HIP;
        HIPCHK(h, hipGraphLaunch(exec, h->stream));
        h->step_host += span;
        t += span;
    }
    h->phase_active = 0;
    // leave the segment count where the next call finds it (no wait: it may see the one before)
    HIPCHK(h, hand_back_segments(h, &d.ctr->S, h->stream));
    return launch_status(h->err);
}

// Batched stand-alone Spatial Pooler run (include/bithtm_hip.h; htm_sp_run.h): n_steps of htm_sp_step over
// a bank in device memory, without the host in the loop.  The launches of one step, in order: htm_sp_step's front and back,
// then the tail launch with the winner rows and / or the step's record (none for a step that neither learns nor records).
static void enqueue_sp_run_step(htm_handle *h, const uint32_t *bank, int n_inputs, int p, int learning, bool recording, int wmode) {
    Dev &d = h->d;
    enqueue_sp_front(h, bank, n_inputs, p, wmode);
    enqueue_sp_back(h, bank, n_inputs, p, 0, EMIT_ALL, false, wmode);
    const int n_learn = learning ? d.k : 0, n_rec = recording ? (d.k + 255) / 256 : 0;
    if (n_learn + n_rec)
        LAUNCH(h, "sp_run_tail", k_sp_run_tail, n_learn + n_rec, 256, d, bank, n_inputs, p, n_learn, recording ? h->d_sp_rec : nullptr);
}

extern "C" int htm_sp_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning,
                          int32_t use_graph, const htm_sp_run_record *rec) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!device_inputs) { h->err = "htm_sp_run: null bank"; return HTM_ERR_ARGUMENT; }
    if (n_inputs < 1 || n_steps < 0) { h->err = "htm_sp_run: n_inputs >= 1 and n_steps >= 0"; return HTM_ERR_ARGUMENT; }
    if (rec) {
        if (rec->struct_bytes != sizeof(htm_sp_run_record)) { h->err = "htm_sp_run: struct_bytes != sizeof(htm_sp_run_record)"; return HTM_ERR_ARGUMENT; }
        if (!rec->active_column && !rec->active_overlap && !rec->active_boosted) { h->err = "htm_sp_run: no record buffer given"; return HTM_ERR_ARGUMENT; }
    }
    // a handle that also owns a Temporal Memory steps both layers together (see htm_sp_step)
    if (h->cfg.enable_tm) { h->err = "htm_sp_run: the handle also has a Temporal Memory; use htm_run"; return HTM_ERR_STATE; }
    if (!h->cfg.enable_sp) { h->err = "htm_sp_run: the handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_sp_run: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REFUSE_ON_VIEW(h, "htm_sp_run");
    REJECT_WHEN_AHEAD(h);
    if (n_steps == 0) return HTM_OK;
    flush_tail(h);
    HIPCHK(h, hipSetDevice(h->device));
    learning = learning ? 1 : 0;
    if (learning) weights_touched(h);
    refresh_exchange_mode(h);
    // (an open htm_sp_phase step is closed as htm_sp_step closes it: the run's first step starts it over)
    if (int rc = close_open_phases(h)) return rc;
    const bool graph = run_schedule(h, n_steps, use_graph).graph, recording = rec != nullptr;
    if (recording) {
        if (!h->d_sp_rec) { if (int rc = dalloc(h, &h->d_sp_rec, 1)) return rc; }
        // the descriptor of this call (not one of the step's launches: htm_profile does not count it)
        hipLaunchKernelGGL(k_sp_run_begin, dim3(1), dim3(64), 0, h->stream, h->d_sp_rec, rec->active_column, rec->active_overlap, rec->active_boosted,
                           (uint32_t)h->step_host, n_steps);
    }
    const int kGraphSteps = h->knob.graph_steps;
    for (int t = 0; t < n_steps;) {
        const int p = (int)(h->step_host & 1), wmode = step_wmode(h);
        if (!graph) {
            enqueue_sp_run_step(h, device_inputs, n_inputs, p, learning, recording, wmode);
            h->step_host += 1;
            t += 1;
            continue;
        }
        // (nothing in a graph depends on the step index: the kernels read it, and with it the bank row, from the counter block.
        // The first select of a handle leaves the window behind that the later ones use: that step is a graph of its own.  Spans
        // start at even steps only: one span graph then serves every call, whatever the parity it starts at)
        const bool settled = h->window_known || !(h->emit_fused && h->knob.step_window);
        const int span = settled && p == 0 && n_steps - t >= kGraphSteps ? kGraphSteps : 1;
        const SpRunGraphKey key{p, learning, recording, h->emit_fused, wmode, span, device_inputs, n_inputs};
        const hipGraphExec_t exec = cached_graph(h->sp_graphs, key, h->stream, h->err, [&] {
            for (int i = 0; i < span; ++i) enqueue_sp_run_step(h, device_inputs, n_inputs, (p + i) & 1, learning, recording, wmode);
            return 0;
        });
        if (!exec) return HTM_ERR_HIP;
        HIPCHK(h, hipGraphLaunch(exec, h->stream));
        h->window_known = true;                     // (as enqueue_sp_back says of the launches the graph replays)
        h->step_host += span;
        t += span;
    }
    return launch_status(h->err);
}

extern "C" int htm_graph_count(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    return (int)std::min<size_t>(h->graphs.size() + h->shard_graphs.size() + h->tm_graphs.size() + h->sp_graphs.size(), 0x7fffffff);
}

extern "C" int htm_run_plan(htm_handle *h, int32_t n_steps, int32_t use_graph) {
    if (!h || n_steps < 0) return HTM_ERR_ARGUMENT;
    if (!h->cfg.enable_sp || !h->cfg.enable_tm || h->world > 1) { h->err = "htm_run_plan: htm_run needs an unsharded handle with SP and TM"; return HTM_ERR_STATE; }
    refresh_exchange_mode(h);
    refresh_seg_hint(h);
    const RunSchedule sched = run_schedule(h, n_steps, use_graph);
    const bool graph = sched.graph, pipeline = sched.pipeline && n_steps > 1;
    return (graph ? HTM_PLAN_GRAPH : 0) | (pipeline ? HTM_PLAN_PIPELINED : 0) | (pipeline && can_lean(h) ? HTM_PLAN_LEAN : 0) |
           (scan_pool_is_large(h) ? HTM_PLAN_SCAN_LARGE : 0);
}

static int read_counters(htm_handle *h, Counters *out);
static int stage_input(htm_handle *h, const uint32_t *packed_input);
static int ensure_shard_buffers(htm_handle *h);

extern "C" int64_t htm_shard_record_bytes(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    return (int64_t)shard_record_bytes(h->d.cand_cap);
}

// front_done: this step's overlap (own columns) was computed beside the previous step's learning and scan (htm_shard_run)
static int shard_enqueue_begin(htm_handle *h, const uint32_t *bank, int n_inputs, void *send_device, bool front_done = false) {
    Dev &d = h->d;
    const int p = (int)(h->step_host & 1);
    d.send = (unsigned char *)send_device;
    // own columns: overlap + boost + histogram (unless computed ahead); the local select's finish, the cell words each
    // candidate would have if it became active, the record -- and, in further blocks of that launch, the zeroing of the step's
    // dense words
    // (the local select: one windowed histogram pass beside the overlap, finished inside the candidates kernel;
    // BITHTM_SHARD_WINDOW=0: two launched digits.  While another handle with a stream of its own is live on the device the
    // blocks of a grid must not wait for each other: every digit by a launch, the counts by k_sp_count -- same candidates)
    const int fused = h->emit_fused ? 1 : 0;
    const int wmode = fused ? h->knob.shard_window : 0;
    if (front_done && h->shard_front_wmode != wmode) {       // the exchange mode changed since the front was computed: start over
        HIPCHK(h, clear_front_hist(h, p));
        front_done = false;
    }
    if (!front_done) LAUNCH(h, "shard_overlap", k_shard_overlap, h->sz.sp_blocks, RB, d, bank, n_inputs, h->sz.G, p, wmode, 0);
    if (!wmode) launch_sel_passes(h, d, p);
    if (!fused) LAUNCH(h, "sp_count", k_sp_count, h->sz.c256_blocks, 256, d, p);
    LAUNCH(h, "shard_candidates", k_sp_emit, h->sz.c256_blocks + std::min((d.C + 255) / 256, 64), 256, d, p, 1, fused, EMIT_LOCAL, wmode, h->sz.c256_blocks);
    return 0;
}

// front_next: compute the coming step's overlap beside this step's learning and scan (same bank: htm_shard_run)
static int shard_enqueue_finish(htm_handle *h, const uint32_t *bank, int n_inputs, const void *recv_device, int learning, bool front_next = false) {
    Dev &d = h->d;
    const int p = (int)(h->step_host & 1);
    LAUNCH(h, "shard_select", k_shard_select, h->world + 1, 1024, d, (const unsigned char *)recv_device, p);      // (+ 1: the death reports)
    const int wmode = h->emit_fused ? h->knob.shard_window : 0;
    enqueue_tm(h, d.k, learning, 1, p, bank, n_inputs, true, front_next ? wmode : -1);
    if (front_next) h->shard_front_wmode = wmode;
    h->step_host += 1;
    return launch_status(h->err);
}

extern "C" int htm_shard_begin(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, const uint32_t *packed_input,
                               int32_t learning, void *send_device) {
    if (!h || !send_device || (!device_inputs == !packed_input)) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_shard_begin");
    if (h->world < 2) { h->err = "htm_shard_begin: handle is not sharded"; return HTM_ERR_STATE; }
    if (h->shard_open) { h->err = "htm_shard_begin: previous step not finished"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    refresh_exchange_mode(h);
    if (packed_input) {
        int rc = stage_input(h, packed_input);
        if (rc) return rc;
        h->shard_bank = h->d.input_stage;
        h->shard_n_inputs = 1;
    } else {
        if (n_inputs < 1) return HTM_ERR_ARGUMENT;
        h->shard_bank = device_inputs;
        h->shard_n_inputs = n_inputs;
    }
    int rc = shard_enqueue_begin(h, h->shard_bank, h->shard_n_inputs, send_device);
    if (rc) return rc;
    h->shard_open = true;
    (void)learning;
    return HTM_OK;
}

extern "C" int htm_shard_finish(htm_handle *h, const void *recv_device, int32_t learning) {
    if (!h || !recv_device) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_shard_finish");
    if (h->world < 2 || !h->shard_open) { h->err = "htm_shard_finish: no step in progress"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    h->shard_open = false;
    return shard_enqueue_finish(h, h->shard_bank, h->shard_n_inputs, recv_device, learning ? 1 : 0);
}

// ---- the exchange inside the library: RCCL, loaded at run time (a handle that is never sharded needs no RCCL) ----
namespace {
struct RcclApi {
    void *lib = nullptr;
    int (*get_unique_id)(void *) = nullptr;
    int (*comm_init_rank)(void **, int, ncclUniqueIdBytes, int) = nullptr;
    int (*all_gather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    int (*comm_count)(void *, int *) = nullptr;
    const char *(*get_error_string)(int) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mutex;

const char *load_rccl() {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.lib) return nullptr;
    void *lib = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
        if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!lib) return "cannot load librccl.so";
    RcclApi api;
    api.lib = lib;
    api.get_unique_id = (int (*)(void *))dlsym(lib, "ncclGetUniqueId");
    api.comm_init_rank = (int (*)(void **, int, ncclUniqueIdBytes, int))dlsym(lib, "ncclCommInitRank");
    api.all_gather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(lib, "ncclAllGather");
    api.comm_destroy = (int (*)(void *))dlsym(lib, "ncclCommDestroy");
    api.get_error_string = (const char *(*)(int))dlsym(lib, "ncclGetErrorString");
    api.comm_count = (int (*)(void *, int *))dlsym(lib, "ncclCommCount");
    if (!api.get_unique_id || !api.comm_init_rank || !api.all_gather || !api.comm_destroy) return "librccl.so lacks an expected symbol";
    g_rccl = api;
    g_rccl_destroy = api.comm_destroy;
    return nullptr;
}
}  // namespace

extern "C" int htm_shard_unique_id(void *out128) {
    if (!out128) return HTM_ERR_ARGUMENT;
    if (const char *err = load_rccl()) { g_create_error = err; return HTM_ERR_HIP; }
    ncclUniqueIdBytes id;
    if (g_rccl.get_unique_id(&id) != 0) { g_create_error = "ncclGetUniqueId failed"; return HTM_ERR_HIP; }
    memcpy(out128, &id, sizeof(id));
    return HTM_OK;
}

extern "C" int htm_keyed_draws(uint32_t seed, int32_t stream, uint32_t step, const uint32_t *a, const uint32_t *b, int64_t n, double *out) {
    if (stream < 1 || stream > 5 || n < 0 || (n && (!a || !out))) return HTM_ERR_ARGUMENT;
    const uint32_t base = htm_stream_base(seed, (uint32_t)stream, step);
    for (int64_t i = 0; i < n; ++i) out[i] = (double)htm_draw24(base, a[i], b ? b[i] : 0u) * (1.0 / 16777216.0);
    return HTM_OK;
}

// RCCL round trip at world size 1 on `device`: load the library, create a communicator, all-gather a buffer on a
// stream, compare, destroy.  What a one-GPU box can verify of the in-library exchange (the symbols, the by-value
// unique id, the call on a non-default stream); returns 0 or a negative status (htm_last_error(NULL)).
extern "C" int htm_rccl_selftest(int32_t device) {
    if (const char *err = load_rccl()) { g_create_error = err; return HTM_ERR_HIP; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return HTM_ERR_HIP; }
    ncclUniqueIdBytes id;
    if (g_rccl.get_unique_id(&id) != 0) { g_create_error = "ncclGetUniqueId failed"; return HTM_ERR_HIP; }
    void *comm = nullptr;
    if (g_rccl.comm_init_rank(&comm, 1, id, 0) != 0) { g_create_error = "ncclCommInitRank failed"; return HTM_ERR_HIP; }
    hipStream_t stream;
    unsigned char *a = nullptr, *b = nullptr;
    const size_t n = 27264;                         // the record of 1311 candidates
    std::vector<unsigned char> src(n), dst(n, 0);
    for (size_t i = 0; i < n; ++i) src[i] = (unsigned char)(i * 131u + 7u);
    bool ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess && hipMalloc((void **)&a, n) == hipSuccess &&
              hipMalloc((void **)&b, n) == hipSuccess && hipMemcpy(a, src.data(), n, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && g_rccl.all_gather(a, b, n, 0, comm, stream) == 0 && hipStreamSynchronize(stream) == hipSuccess &&
         hipMemcpy(dst.data(), b, n, hipMemcpyDeviceToHost) == hipSuccess && dst == src;
    // and the same collective captured into a hipGraph and replayed (what htm_shard_run does with whole timesteps)
    int captured = 0;
    if (ok) {
        hipGraph_t graph_obj = nullptr;
        hipGraphExec_t exec = nullptr;
        std::fill(dst.begin(), dst.end(), 0);
        bool cap = hipMemset(b, 0, n) == hipSuccess && hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (cap) {
            const bool in = g_rccl.all_gather(a, b, n, 0, comm, stream) == 0;
            cap = hipStreamEndCapture(stream, &graph_obj) == hipSuccess && in && graph_obj &&
                  hipGraphInstantiate(&exec, graph_obj, nullptr, nullptr, 0) == hipSuccess;
        }
        if (cap) cap = hipGraphLaunch(exec, stream) == hipSuccess && hipStreamSynchronize(stream) == hipSuccess &&
                       hipMemcpy(dst.data(), b, n, hipMemcpyDeviceToHost) == hipSuccess && dst == src;
        if (exec) hipGraphExecDestroy(exec);
        if (graph_obj) hipGraphDestroy(graph_obj);
        (void)hipGetLastError();
        captured = cap ? 1 : 0;
    }
    g_rccl.comm_destroy(comm);
    if (a) hipFree(a);
    if (b) hipFree(b);
    hipStreamDestroy(stream);
    if (!ok) { g_create_error = "RCCL all-gather self-test failed"; return HTM_ERR_HIP; }
    return captured ? HTM_OK : 1;                   // 1: the collective works but this runtime does not capture it (htm_shard_run then launches eagerly)
}

extern "C" int htm_shard_comm_init(htm_handle *h, const void *unique_id128) {
    if (!h || !unique_id128) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_shard_comm_init");
    if (h->world < 2) { h->err = "htm_shard_comm_init: handle is not sharded"; return HTM_ERR_STATE; }
    if (h->rccl_comm) { h->err = "htm_shard_comm_init: already initialised"; return HTM_ERR_STATE; }
    if (const char *err = load_rccl()) { h->err = err; return HTM_ERR_HIP; }
    HIPCHK(h, hipSetDevice(h->device));
    ncclUniqueIdBytes id;
    memcpy(&id, unique_id128, sizeof(id));
    void *comm = nullptr;
    const int rc = g_rccl.comm_init_rank(&comm, h->world, id, h->rank);
    if (rc != 0) { h->err = std::string("ncclCommInitRank: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(rc) : "failed"); return HTM_ERR_HIP; }
    h->rccl_comm = comm;
    int rc2 = ensure_shard_buffers(h);
    if (rc2) return rc2;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // Preflight on THIS communicator and THESE buffers, collectively (every rank runs the same two gathers): the exchange of a
    // timestep launched eagerly -- its result checked: rank q's part of the gathered buffer must hold q's pattern -- and the same
    // collective captured into a hipGraph and replayed.  htm_shard_run replays whole timesteps as graphs only if the second
    // check passes here (a rank that launches eagerly and one that replays issue the same collective: the modes may differ).
    {
        const size_t rb = shard_record_bytes(h->d.cand_cap);
        std::vector<unsigned char> got(rb * (size_t)h->world);
        auto check = [&]() -> bool {
            if (hipStreamSynchronize(h->stream) != hipSuccess || hipMemcpy(got.data(), h->shard_recv, got.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
            for (int q = 0; q < h->world; ++q)
                for (size_t i = 0; i < rb; i += 997)
                    if (got[(size_t)q * rb + i] != (unsigned char)(q + 1)) return false;
            return true;
        };
        HIPCHK(h, hipMemsetAsync(h->shard_send, h->rank + 1, rb, h->stream));
        HIPCHK(h, hipMemsetAsync(h->shard_recv, 0, rb * (size_t)h->world, h->stream));
        // (a rank whose first gather fails still issues the second: its peers are on their way into theirs and would wait for
        // it for ever; the failure is reported after both)
        int nrc = g_rccl.all_gather(h->shard_send, h->shard_recv, rb, 0, comm, h->stream);
        const bool first_ok = nrc == 0 && check();
        bool ok = first_ok && h->stream != nullptr && hipMemsetAsync(h->shard_recv, 0, rb * (size_t)h->world, h->stream) == hipSuccess &&
                  hipStreamSynchronize(h->stream) == hipSuccess;      // (the default stream cannot be captured)
        hipGraph_t graph_obj = nullptr;
        hipGraphExec_t exec = nullptr;
        if (ok && hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const bool in = g_rccl.all_gather(h->shard_send, h->shard_recv, rb, 0, comm, h->stream) == 0;
            ok = hipStreamEndCapture(h->stream, &graph_obj) == hipSuccess && in && graph_obj && hipGraphInstantiate(&exec, graph_obj, nullptr, nullptr, 0) == hipSuccess;
        } else {
            ok = false;
        }
        // (every rank must issue the second gather, captured or not: the others are waiting in theirs)
        if (ok) ok = hipGraphLaunch(exec, h->stream) == hipSuccess;
        else ok = g_rccl.all_gather(h->shard_send, h->shard_recv, rb, 0, comm, h->stream) == 0 && false;
        const bool delivered = check();
        if (exec) hipGraphExecDestroy(exec);
        if (graph_obj) hipGraphDestroy(graph_obj);
        (void)hipGetLastError();
        h->shard_graph_ok = ok && delivered;
        HIPCHK(h, hipMemsetAsync(h->shard_send, 0, rb, h->stream));
        HIPCHK(h, hipMemsetAsync(h->shard_recv, 0, rb * (size_t)h->world, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        if (!first_ok) { h->err = "htm_shard_comm_init: the all-gather over this communicator does not deliver the ranks' records"; return HTM_ERR_HIP; }
    }
    return HTM_OK;
}

// 1: htm_shard_run replays whole timesteps (the all-gather included) as hipGraphs on this handle; 0: it launches eagerly
// (the preflight of htm_shard_comm_init found the collective not capturable, or the handle enqueues on the default stream)
extern "C" int htm_shard_graph_ok(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    return h->shard_graph_ok ? 1 : 0;
}

// ranks of the RCCL communicator htm_shard_step / htm_shard_run exchange over (ncclCommCount): what a scaling run reports
extern "C" int htm_shard_comm_size(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!h->rccl_comm || !g_rccl.comm_count) { h->err = "htm_shard_comm_size: no communicator (htm_shard_comm_init)"; return HTM_ERR_STATE; }
    int n = 0;
    if (g_rccl.comm_count(h->rccl_comm, &n) != 0) { h->err = "ncclCommCount failed"; return HTM_ERR_HIP; }
    return n;
}

static int ensure_shard_buffers(htm_handle *h) {
    if (h->shard_send) return 0;
    const size_t rb = shard_record_bytes(h->d.cand_cap);
    int rc = dalloc(h, &h->shard_send, rb);
    rc |= dalloc(h, &h->shard_recv, rb * (size_t)h->world);
    return rc;
}

// All the shards of a model inside ONE process on one device (tests, single-GPU rehearsals, bench.py's configs[4]
// leg): handles[r] is rank r of n = shard_world, all of them on the same stream; the all-gather is n x n device copies.
extern "C" int htm_shard_group_step(htm_handle *const *handles, int32_t n, const uint32_t *const *device_inputs, int32_t n_inputs,
                                    const uint32_t *packed_input, int32_t learning) {
    if (!handles || n < 2 || (!device_inputs == !packed_input)) return HTM_ERR_ARGUMENT;
    for (int r = 0; r < n; ++r) {
        htm_handle *h = handles[r];
        if (!h || h->world != n || h->rank != r || h->stream != handles[0]->stream || h->device != handles[0]->device) {
            if (h) h->err = "htm_shard_group_step: handles must be ranks 0..n-1 of one group on one stream";
            return HTM_ERR_ARGUMENT;
        }
    }
    for (int r = 0; r < n; ++r) {
        htm_handle *h = handles[r];
        HIPCHK(h, hipSetDevice(h->device));
        refresh_exchange_mode(h);
        int rc = ensure_shard_buffers(h);
        if (rc) return rc;
        const uint32_t *bank = device_inputs ? device_inputs[r] : nullptr;
        if (packed_input) {
            rc = stage_input(h, packed_input);
            if (rc) return rc;
            bank = h->d.input_stage;
        }
        h->shard_bank = bank;
        h->shard_n_inputs = packed_input ? 1 : n_inputs;
        rc = shard_enqueue_begin(h, h->shard_bank, h->shard_n_inputs, h->shard_send);
        if (rc) return rc;
    }
    const size_t rb = shard_record_bytes(handles[0]->d.cand_cap);
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < n; ++q)
            HIPCHK(handles[r], hipMemcpyAsync(handles[r]->shard_recv + (size_t)q * rb, handles[q]->shard_send, rb, hipMemcpyDeviceToDevice, handles[r]->stream));
    for (int r = 0; r < n; ++r) {
        int rc = shard_enqueue_finish(handles[r], handles[r]->shard_bank, handles[r]->shard_n_inputs, handles[r]->shard_recv, learning ? 1 : 0);
        if (rc) return rc;
    }
    return HTM_OK;
}

extern "C" int htm_shard_step(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, const uint32_t *packed_input, int32_t learning) {
    if (!h || (!device_inputs == !packed_input)) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_shard_step");
    if (h->world < 2 || !h->rccl_comm) { h->err = "htm_shard_step: needs a sharded handle after htm_shard_comm_init"; return HTM_ERR_STATE; }
    if (h->shard_open) { h->err = "htm_shard_step: a step opened with htm_shard_begin is not finished"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    refresh_exchange_mode(h);
    const uint32_t *bank = device_inputs;
    if (packed_input) {
        int rc = stage_input(h, packed_input);
        if (rc) return rc;
        bank = h->d.input_stage;
        n_inputs = 1;
    } else if (n_inputs < 1) {
        return HTM_ERR_ARGUMENT;
    }
    int rc = shard_enqueue_begin(h, bank, n_inputs, h->shard_send);
    if (rc) return rc;
    const size_t rb = shard_record_bytes(h->d.cand_cap);
    const int nrc = g_rccl.all_gather(h->shard_send, h->shard_recv, rb, /* ncclChar */ 0, h->rccl_comm, h->stream);
    if (nrc != 0) { h->err = std::string("ncclAllGather: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(nrc) : "failed"); return HTM_ERR_HIP; }
    return shard_enqueue_finish(h, bank, n_inputs, h->shard_recv, learning ? 1 : 0);
}

// ---- n timesteps of the column-sharded step without the host in the loop (htm_shard_run, htm_shard_group_run) ----
// Inside a run the overlap of step t + 1 (own columns) rides in the last launch of step t, and the launches of whole
// steps -- the collective included: RCCL's all-gather is captured like a kernel -- are replayed as hipGraphs (two parities
// per graph, up to 16 steps).  hs = the handles stepped together (one: this process's rank, the exchange by RCCL;
// several: all ranks of a group in one process, the exchange as device copies).
static int shard_exchange(htm_handle *const *hs, int n) {
    if (n == 1) {
        htm_handle *h = hs[0];
        const int nrc = g_rccl.all_gather(h->shard_send, h->shard_recv, shard_record_bytes(h->d.cand_cap), /* ncclChar */ 0, h->rccl_comm, h->stream);
        if (nrc != 0) { h->err = std::string("ncclAllGather: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(nrc) : "failed"); return HTM_ERR_HIP; }
        return 0;
    }
    const size_t rb = shard_record_bytes(hs[0]->d.cand_cap);
    for (int r = 0; r < n; ++r)
        for (int q = 0; q < n; ++q)
            HIPCHK(hs[r], hipMemcpyAsync(hs[r]->shard_recv + (size_t)q * rb, hs[q]->shard_send, rb, hipMemcpyDeviceToDevice, hs[r]->stream));
    return 0;
}

// `count` consecutive steps; first_front_done: the first one's overlap exists already; last_front_next: the last one
// computes the overlap of the step after it
static int shard_enqueue_steps(htm_handle *const *hs, int n, const uint32_t *const *banks, int n_inputs, int learning, int count,
                               bool first_front_done, bool last_front_next) {
    for (int i = 0; i < count; ++i) {
        const bool fd = i > 0 || first_front_done, fn = i + 1 < count || last_front_next;
        for (int r = 0; r < n; ++r) {
            int rc = shard_enqueue_begin(hs[r], banks[r], n_inputs, hs[r]->shard_send, fd);
            if (rc) return rc;
        }
        int rc = shard_exchange(hs, n);
        if (rc) return rc;
        for (int r = 0; r < n; ++r) {
            rc = shard_enqueue_finish(hs[r], banks[r], n_inputs, hs[r]->shard_recv, learning, fn);
            if (rc) return rc;
        }
    }
    return 0;
}

static int shard_run(htm_handle *const *hs, int n, const uint32_t *const *banks, int n_inputs, int n_steps, int learning, int use_graph) {
    htm_handle *h0 = hs[0];
    learning = learning ? 1 : 0;
    bool pipeline = !(use_graph & 2), graph = (use_graph & 1) != 0;
    for (int r = 0; r < n; ++r) {
        htm_handle *h = hs[r];
        HIPCHK(h, hipSetDevice(h->device));
        refresh_exchange_mode(h);
        int rc = ensure_shard_buffers(h);
        if (rc) return rc;
        refresh_seg_hint(h);
        if (h->profile) graph = false;
    }
    if (n == 1 && !h0->shard_graph_ok) graph = false;      // (this communicator's collective does not replay from a graph: the preflight said so)
    const int kSpan = 16;
    for (int t = 0; t < n_steps;) {
        // steady state: steps whose overlap was computed ahead and that compute the next one's; the first and the last step
        // of a call are launched on their own
        const bool fd = pipeline && t > 0, steady = fd && t + 1 < n_steps;
        int span = 1;
        if (steady && graph) span = std::min(kSpan, (n_steps - 1 - t) & ~1) > 0 ? std::min(kSpan, (n_steps - 1 - t) & ~1) : 1;
        const bool fn = pipeline && t + span < n_steps;
        if (!graph) {
            int rc = shard_enqueue_steps(hs, n, banks, n_inputs, learning, span, fd, fn);
            if (rc) return rc;
            t += span;
            continue;
        }
        ShardGraphKey key{(int)(h0->step_host & 1), learning, fd, fn, span, n, n_inputs, {}, banks[0]};
        for (int r = 0; r < n; ++r)             // what the launches of a rank depend on besides its arguments
            key.per_rank.emplace_back(scan_spec_blocks(hs[r]), scan_pool_is_large(hs[r]), hs[r]->emit_fused);
        const hipGraphExec_t exec = cached_graph(h0->shard_graphs, key, h0->stream, h0->err, [&] {
            std::vector<long long> saved((size_t)n);
            for (int r = 0; r < n; ++r) saved[(size_t)r] = hs[r]->step_host;
            const int rc = shard_enqueue_steps(hs, n, banks, n_inputs, learning, span, fd, fn);
            for (int r = 0; r < n; ++r) hs[r]->step_host = saved[(size_t)r];      // (captured, not run)
            return rc;
        });
        if (!exec) {                                // (a collective that cannot be captured on this runtime: launch eagerly from here on)
            (void)hipGetLastError();
            graph = false;
            h0->err.clear();
            continue;
        }
        HIPCHK(h0, hipGraphLaunch(exec, h0->stream));
        for (int r = 0; r < n; ++r) hs[r]->step_host += span;
        t += span;
    }
    if (n_steps > 0)
        for (int r = 0; r < n; ++r)
            HIPCHK(hs[r], hand_back_segments(hs[r], &hs[r]->d.ctr->L, hs[r]->stream));
    return HTM_OK;
}

extern "C" int htm_shard_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning, int32_t use_graph) {
    if (!h || !device_inputs || n_inputs < 1 || n_steps < 0) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_shard_run");
    if (h->world < 2 || !h->rccl_comm) { h->err = "htm_shard_run: needs a sharded handle after htm_shard_comm_init"; return HTM_ERR_STATE; }
    if (h->shard_open) { h->err = "htm_shard_run: a step opened with htm_shard_begin is not finished"; return HTM_ERR_STATE; }
    htm_handle *hs[1] = {h};
    const uint32_t *banks[1] = {device_inputs};
    return shard_run(hs, 1, banks, n_inputs, n_steps, learning, use_graph);
}

extern "C" int htm_shard_group_run(htm_handle *const *handles, int32_t n, const uint32_t *const *device_inputs, int32_t n_inputs, int32_t n_steps,
                                   int32_t learning, int32_t use_graph) {
    if (!handles || n < 2 || !device_inputs || n_inputs < 1 || n_steps < 0) return HTM_ERR_ARGUMENT;
    for (int r = 0; r < n; ++r) {
        htm_handle *h = handles[r];
        if (!h || h->world != n || h->rank != r || h->stream != handles[0]->stream || h->device != handles[0]->device || !device_inputs[r]) {
            if (h) h->err = "htm_shard_group_run: handles must be ranks 0..n-1 of one group on one stream, each with its bank";
            return HTM_ERR_ARGUMENT;
        }
    }
    return shard_run(handles, n, device_inputs, n_inputs, n_steps, learning, use_graph);
}

// Pre-populated pool (BASELINE.json configs[4]: a pure scan stress, not a learned state): every cell with flat id in
// [cell_begin, cell_end) gets segments_per_cell segments of `synapses` synapses to keyed-random presynaptic cells
// (no two alike within a segment), permanences keyed-uniform in [perm_lo, perm_hi).  Segment ids are cell-major:
// (cell - cell_begin) * segments_per_cell + j.  Generated on the device (oracle twin: TemporalMemoryOracle.populate);
// a column-sharded handle generates the rows of its own cells only, every handle of the group is given the same range.
extern "C" int htm_populate(htm_handle *h, int64_t cell_begin, int64_t cell_end, int32_t segments_per_cell, int32_t synapses,
                            double perm_lo, double perm_hi, uint32_t seed) {
    if (!h) return HTM_ERR_ARGUMENT;
    REFUSE_ON_VIEW(h, "htm_populate");
    weights_touched(h);
    if (h) flush_tail(h);
    if (!h->cfg.enable_tm) { h->err = "handle has no Temporal Memory"; return HTM_ERR_STATE; }
    Dev &d = h->d;
    const int64_t N = (int64_t)d.C * d.K;
    if (cell_begin < 0 || cell_end > N || cell_begin > cell_end || segments_per_cell < 1 || synapses < d.match_thr || synapses > 64 ||
        synapses > d.E || synapses > N || !(perm_lo >= 0.0) || !(perm_hi >= perm_lo)) { h->err = "htm_populate: bad arguments"; return HTM_ERR_ARGUMENT; }
    Counters c;
    int rc = read_counters(h, &c);
    if (rc) return rc;
    if (c.S != 0 || h->step_host != 0) { h->err = "htm_populate: the handle must be fresh"; return HTM_ERR_STATE; }
    const int64_t total = (cell_end - cell_begin) * segments_per_cell;
    const int64_t own_lo = std::max<int64_t>(cell_begin, (int64_t)d.c0 * d.K), own_hi = std::min<int64_t>(cell_end, (int64_t)d.c1 * d.K);
    const int64_t own = std::max<int64_t>(own_hi - own_lo, 0) * segments_per_cell;
    if (total > d.Scap || own > d.Lcap) { h->err = "htm_populate: pool too small (segment_capacity / segment_capacity_local)"; return HTM_ERR_CAPACITY; }
    if (own > 0) {
        const int64_t blocks = std::min<int64_t>((own + 3) / 4, (int64_t)h->sz.cus * 64);
        hipLaunchKernelGGL(k_tm_populate, dim3((unsigned)blocks), dim3(256), 0, h->stream, d, (long long)cell_begin, (long long)own_lo, (long long)own,
                           segments_per_cell, synapses, perm_lo, perm_hi, seed);
    }
    c.S = (int32_t)total;
    c.L = (int32_t)own;
    HIPCHK(h, hipMemcpyAsync(&d.ctr->S, &c.S, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(&d.ctr->L, &c.L, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->seg_hint = (int)(h->world > 1 ? own : total);
    if (h->seg_pinned) *h->seg_pinned = h->seg_hint;
    return HTM_OK;
}

extern "C" int htm_bank_upload(htm_handle *h, const uint32_t *host_inputs, int32_t n_inputs, uint32_t **device_bank) {
    if (!h || !host_inputs || n_inputs < 1 || !device_bank) return HTM_ERR_ARGUMENT;
    if (!h->cfg.enable_sp) { h->err = "handle has no Spatial Pooler"; return HTM_ERR_STATE; }
    Dev &d = h->d;
    HIPCHK(h, hipSetDevice(h->device));
    uint32_t *bank = nullptr;
    int rc = dalloc(h, &bank, (size_t)n_inputs * d.W);
    if (rc) return rc;
    const size_t words = (size_t)(d.I + 31) / 32;
    HIPCHK(h, hipMemcpy2DAsync(bank, (size_t)d.W * 4, host_inputs, words * 4, words * 4, (size_t)n_inputs,
                               hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *device_bank = bank;
    return HTM_OK;
}

static int read_counters(htm_handle *h, Counters *out) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->d.ctr, sizeof(Counters), hipMemcpyDeviceToHost));
    h->seg_hint = h->world > 1 ? out->L : out->S;   // exact: the stream is idle (rows the scan covers)
    if (h->seg_pinned) *h->seg_pinned = h->seg_hint;
    return 0;
}

extern "C" int htm_get_info(htm_handle *h, htm_info *out) {
    if (!h || !out) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    Counters c;
    int rc = read_counters(h, &c);
    if (rc) return rc;
    const int q = (int)((h->step_host + 1) & 1);          // parity of the last completed step
    const int rows = h->world > 1 ? c.L : c.S;
    out->step_index = h->step_host;
    out->segments = c.S;
    out->local_segments = rows;
    out->matching_segments = 0;
    if (c.has_distal && rows > 0) {
        std::vector<uint32_t> bits(((size_t)rows + 31) / 32);
        HIPCHK(h, hipMemcpy(bits.data(), h->d.match_bits[q], bits.size() * 4, hipMemcpyDeviceToHost));
        for (int i = 0; i < rows; ++i) out->matching_segments += (bits[(size_t)i >> 5] >> (i & 31)) & 1u;
    }
    out->winner_cells = c.n_win[q];
    out->active_cells = c.n_active_cells;
    out->has_distal_state = c.has_distal;
    out->has_winner_cells = h->step_host > 0 ? c.has_winner[q] : 0;
    out->capacity_error = c.error;
    out->words_per_row = h->d.W;
    out->new_segment_requests = c.n_un;
    out->recycled_segments = c.n_un ? c.n_recycled : 0;
    out->appended_segments = c.n_un ? c.n_new : 0;
    out->work_items = c.n_work_last;
    out->select_fallbacks = c.sel_fallbacks;
    out->candidate_exact_steps = c.cand_exact;
    out->hot_select_steps = c.hot_selects;
    out->select_zoom_steps = c.sel_zooms;
    if (c.error) {
        h->err = std::string("capacity exhausted:") + ((c.error & 1) ? " segment pool (segment_capacity)" : "") +
                 ((c.error & 2) ? " synapse slots (segment_slots)" : "") + ((c.error & 4) ? " work list / growth staging" : "") +
                 ((c.error & 8) ? " dead-segment report (DEAD_CAP)" : "") +
                 ((c.error & 16) ? " (internal) block hand-off timed out in k_sp_emit" : "") +
                 ((c.error & 32) ? " (internal) the middle role's wait for the activation blocks timed out in k_act_mid_rows" : "") +
                 ((c.error & 64) ? " (not a capacity) htm_pack_columns met a column id outside this handle's input range" : "") +
                 ((c.error & 128) ? " (not a capacity) htm_tm_run met a list row with a repeated column id or one outside [0, column_dim): the results of its steps are invalid" : "");
        return HTM_ERR_CAPACITY;          // *out is filled in all the same
    }
    return HTM_OK;
}

// conversions between the internal cell encoding (col * KP + cell: 32 cell slots per column, 64 for cell_dim above 32) and the
// ABI's flat ids
static inline int enc_flat(int enc, int K) { return K > 32 ? (enc >> 6) * K + (enc & 63) : (enc >> 5) * K + (enc & 31); }
static inline int flat_enc(int flat, int K) { return (flat / K) * (K > 32 ? 64 : 32) + (flat % K); }

extern "C" int64_t htm_read(htm_handle *h, int32_t field, void *dst, int64_t count) {
    if (!h || !dst) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    // the fields whose length the handle's shape gives need no counters: the stream is waited for, nothing else (a State of the
    // reference's API is a dozen reads, and the counters' copy was half of each small one)
    const bool fixed_size = field == HTM_F_ACTIVE_COLUMN || field == HTM_F_OVERLAPS || field == HTM_F_BOOSTED || field == HTM_F_DUTY_CYCLE ||
                            field == HTM_F_CELL_ACTIVATION || field == HTM_F_CELL_PREDICTION || field == HTM_F_WINNER_WORDS ||
                            field == HTM_F_BURSTING || field == HTM_F_SEGCOUNT || field == HTM_F_CELL_MAX_JITTER;
    Counters c;
    memset(&c, 0, sizeof(c));
    int rc = 0;
    if (fixed_size) {
        HIPCHK(h, hipSetDevice(h->device));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    } else {
        rc = read_counters(h, &c);
        if (rc) return rc;
    }
    Dev &d = h->d;
    const int q = (int)((h->step_host + 1) & 1);
    const int qs = h->phase_open ? (int)(h->step_host & 1) : q;      // Spatial Pooler fields while a step is run phase by phase
    const bool sp = h->cfg.enable_sp, tm = h->cfg.enable_tm;
    const int64_t C = d.C, K = d.K, S = h->world > 1 ? c.L : c.S, E = d.E, CW = (int64_t)d.C * d.WPC, KP = d.KP;      // S: rows of the per-segment fields; CW: cell words
    auto need = [&](bool ok, int64_t n) -> int64_t {
        if (!ok) { h->err = "htm_read: field not available on this handle"; return HTM_ERR_STATE; }
        if (count < n) { h->err = "htm_read: buffer too small"; return HTM_ERR_ARGUMENT; }
        return n;
    };
    auto copy = [&](const void *src, int64_t n, size_t elem) -> int64_t {
        if (n > 0 && hipMemcpy(dst, src, (size_t)n * elem, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read: hipMemcpy failed"; return HTM_ERR_HIP; }
        return n;
    };
    int64_t n;
    switch (field) {
        case HTM_F_ACTIVE_COLUMN: if ((n = need(true, d.k)) < 0) return n; return copy(d.active_cols[qs], n, 4);
        case HTM_F_OVERLAPS: REJECT_WHEN_AHEAD(h); if ((n = need(sp, C)) < 0) return n; return copy(d.overlap[qs], n, 4);
        case HTM_F_BOOSTED: REJECT_WHEN_AHEAD(h); if ((n = need(sp, C)) < 0) return n; return copy(d.boosted[qs], n, 8);
        case HTM_F_DUTY_CYCLE: REJECT_WHEN_AHEAD(h); if ((n = need(sp, C)) < 0) return n; return copy(d.duty, n, 4);
        case HTM_F_CELL_ACTIVATION: if ((n = need(tm, CW)) < 0) return n; return copy(d.act[q], n, 4);
        case HTM_F_CELL_PREDICTION: if ((n = need(tm, CW)) < 0) return n; return copy(d.pred[q], n, 4);
        case HTM_F_WINNER_WORDS: if ((n = need(tm, CW)) < 0) return n; return copy(d.win[q], n, 4);
        case HTM_F_BURSTING: if ((n = need(tm, d.k)) < 0) return n; return copy(d.bursting, n, 1);
        case HTM_F_SEG_NSYN: if ((n = need(tm, S)) < 0) return n; return copy(d.seg_nsyn, n, 4);
        case HTM_F_SEG_POTENTIAL:
        case HTM_F_MATCH_SEGMENT:
        case HTM_F_MATCH_INFO:
        case HTM_F_MATCH_JITTER: {
            // the device keeps one info word per segment; the matching-segment lists of
            // PredictiveProjection.State (ascending ids, projections.py:247) are its non-zero part
            if (!tm) { h->err = "htm_read: field not available on this handle"; return HTM_ERR_STATE; }
            if (field == HTM_F_SEG_POTENTIAL) {
                // the device keeps the potential of matching segments only: recompute all of them from the
                // last step's activation (same definition, projections.py:175-178 / :246)
                if ((n = need(true, S)) < 0) return n;
                if (S == 0) return 0;
                if (!c.has_distal) { memset(dst, 0, (size_t)S * 4); return S; }
                int *tmp = nullptr;
                if (hipMalloc((void **)&tmp, (size_t)S * 4) != hipSuccess) { h->err = "htm_read: hipMalloc failed"; return HTM_ERR_HIP; }
                hipLaunchKernelGGL(k_tm_potentials, dim3((unsigned)std::min<int64_t>((S * 8 + 255) / 256, 8192)), dim3(256), 0, h->stream, d, q, tmp, 0, (int)S);
                const bool ok = hipStreamSynchronize(h->stream) == hipSuccess && hipMemcpy(dst, tmp, (size_t)S * 4, hipMemcpyDeviceToHost) == hipSuccess;
                hipFree(tmp);
                if (!ok) { h->err = "htm_read: potentials kernel failed"; return HTM_ERR_HIP; }
                return S;
            }
            // one bit per segment says whether it is matching; info word and jitter exist for those only.  The
            // matching-segment lists of PredictiveProjection.State (ascending ids, projections.py:247):
            std::vector<uint32_t> bits(((size_t)S + 31) / 32, 0u);
            std::vector<uint32_t> info((size_t)S);
            std::vector<float> jit((size_t)S);
            if (S && c.has_distal && (hipMemcpy(bits.data(), d.match_bits[q], bits.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                                      hipMemcpy(info.data(), d.seg_info, (size_t)S * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                                      hipMemcpy(jit.data(), d.seg_jit, (size_t)S * 4, hipMemcpyDeviceToHost) != hipSuccess)) { h->err = "htm_read: hipMemcpy failed"; return HTM_ERR_HIP; }
            auto is_matching = [&](int64_t i) { return (bits[(size_t)i >> 5] >> (i & 31)) & 1u; };
            int64_t m = 0;
            for (int64_t i = 0; i < S; ++i) m += is_matching(i);
            if ((n = need(true, m)) < 0) return n;
            m = 0;
            for (int64_t i = 0; i < S; ++i) {
                if (!is_matching(i)) continue;
                const uint32_t v = info[(size_t)i];
                if (field == HTM_F_MATCH_SEGMENT) ((int *)dst)[m] = (int)i;
                else if (field == HTM_F_MATCH_INFO) ((uint32_t *)dst)[m] = v & ~0x40000000u;
                else ((float *)dst)[m] = jit[(size_t)i];
                ++m;
            }
            return m;
        }
        case HTM_F_WINNER_CELL:
        case HTM_F_SEG_CELL: {
            const bool w = field == HTM_F_WINNER_CELL;
            if ((n = need(tm, w ? c.n_win[q] : S)) < 0) return n;
            if ((rc = (int)copy(w ? d.winners[q] : d.seg_cell, n, 4)) < 0) return rc;
            int *v = (int *)dst;
            for (int64_t i = 0; i < n; ++i) v[i] = enc_flat(v[i], (int)K);
            return n;
        }
        case HTM_F_SEG_PRESYN:
        case HTM_F_SEG_PERM: {
            if ((n = need(tm, S * E)) < 0) return n;
            std::vector<int> nsyn((size_t)S);
            if (S && hipMemcpy(nsyn.data(), d.seg_nsyn, (size_t)S * 4, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read: hipMemcpy failed"; return HTM_ERR_HIP; }
            if ((rc = (int)copy(field == HTM_F_SEG_PRESYN ? (const void *)d.presyn : (const void *)d.sperm, n, 4)) < 0) return rc;
            for (int64_t s = 0; s < S; ++s)
                for (int64_t e = 0; e < E; ++e) {
                    const bool valid = e < nsyn[(size_t)s];
                    if (field == HTM_F_SEG_PRESYN) { int *v = (int *)dst + s * E + e; *v = valid ? enc_flat(*v & SYN_CELL, (int)K) : -1; }   // (without the connected flag)
                    else if (!valid) ((float *)dst)[s * E + e] = -1.0f;
                }
            return n;
        }
        case HTM_F_SEGCOUNT:
        case HTM_F_CELL_MAX_JITTER: {
            if ((n = need(tm, C * K)) < 0) return n;
            std::vector<uint32_t> tmp((size_t)C * KP);
            const void *src = field == HTM_F_SEGCOUNT ? (const void *)d.segcount : (const void *)d.cellmax[q];
            if (hipMemcpy(tmp.data(), src, tmp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read: hipMemcpy failed"; return HTM_ERR_HIP; }
            uint32_t *v = (uint32_t *)dst;
            for (int64_t col = 0; col < C; ++col)
                for (int64_t j = 0; j < K; ++j) v[col * K + j] = tmp[(size_t)col * KP + j];
            return n;
        }
        case HTM_F_SEG_GID: {
            if ((n = need(tm, S)) < 0) return n;
            if (d.seg_gid) return copy(d.seg_gid, n, 4);
            for (int64_t i = 0; i < n; ++i) ((int *)dst)[i] = (int)i;
            return n;
        }
        case HTM_F_RECYCLABLE_COUNTS: {
            // the allocation's own books: recyclable segments per 1 024 ids, then per 2^20 ids (read-only; a column-sharded
            // handle keeps dead bits per id instead)
            if (h->world > 1) { h->err = "htm_read: the recyclable counts are not available on a column-sharded handle"; return HTM_ERR_STATE; }
            const int64_t nb = ((int64_t)c.S + 1023) / 1024, nb2 = (nb + 1023) / 1024;
            if ((n = need(tm, nb + nb2)) < 0) return n;
            if (nb && (hipMemcpy(dst, d.recyc_cnt, (size_t)nb * 4, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy((int *)dst + nb, d.recyc_cnt2, (size_t)nb2 * 4, hipMemcpyDeviceToHost) != hipSuccess)) { h->err = "htm_read: hipMemcpy failed"; return HTM_ERR_HIP; }
            return n;
        }
        default: h->err = "htm_read: unknown field"; return HTM_ERR_ARGUMENT;
    }
}

// Rows [row_begin, row_begin + row_count) of a per-segment field: what htm_read returns for the whole pool, for a pool
// too large to read whole (configs[4]: 134 M rows).  HTM_F_MATCH_INFO comes back dense: one word per row, 0 = the row is
// not matching.
extern "C" int64_t htm_read_rows(htm_handle *h, int32_t field, int64_t row_begin, int64_t row_count, void *dst, int64_t count) {
    if (!h || !dst || row_begin < 0 || row_count < 0) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    if (!h->cfg.enable_tm) { h->err = "htm_read_rows: handle has no Temporal Memory"; return HTM_ERR_STATE; }
    Counters c;
    int rc = read_counters(h, &c);
    if (rc) return rc;
    Dev &d = h->d;
    const int q = (int)((h->step_host + 1) & 1);
    const int64_t S = h->world > 1 ? c.L : c.S, E = d.E, K = d.K;
    if (row_begin + row_count > S) { h->err = "htm_read_rows: rows out of range"; return HTM_ERR_ARGUMENT; }
    const int64_t per = (field == HTM_F_SEG_PRESYN || field == HTM_F_SEG_PERM) ? E : 1, n = row_count * per;
    if (count < n) { h->err = "htm_read_rows: buffer too small"; return HTM_ERR_ARGUMENT; }
    if (n == 0) return 0;
    auto copy = [&](const void *src, size_t bytes) -> bool {
        if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read_rows: hipMemcpy failed"; return false; }
        return true;
    };
    switch (field) {
        case HTM_F_SEG_NSYN: return copy(d.seg_nsyn + row_begin, (size_t)n * 4) ? n : HTM_ERR_HIP;
        case HTM_F_SEG_GID: {
            if (d.seg_gid) return copy(d.seg_gid + row_begin, (size_t)n * 4) ? n : HTM_ERR_HIP;
            for (int64_t i = 0; i < n; ++i) ((int *)dst)[i] = (int)(row_begin + i);
            return n;
        }
        case HTM_F_SEG_CELL: {
            if (!copy(d.seg_cell + row_begin, (size_t)n * 4)) return HTM_ERR_HIP;
            for (int64_t i = 0; i < n; ++i) ((int *)dst)[i] = enc_flat(((int *)dst)[i], (int)K);
            return n;
        }
        case HTM_F_SEG_PRESYN:
        case HTM_F_SEG_PERM: {
            std::vector<int> nsyn((size_t)row_count);
            if (hipMemcpy(nsyn.data(), d.seg_nsyn + row_begin, (size_t)row_count * 4, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read_rows: hipMemcpy failed"; return HTM_ERR_HIP; }
            if (!copy(field == HTM_F_SEG_PRESYN ? (const void *)(d.presyn + row_begin * E) : (const void *)(d.sperm + row_begin * E), (size_t)n * 4)) return HTM_ERR_HIP;
            for (int64_t s = 0; s < row_count; ++s)
                for (int64_t e = 0; e < E; ++e) {
                    const bool valid = e < (nsyn[(size_t)s] & ~(int)SEG_BUSY);
                    if (field == HTM_F_SEG_PRESYN) { int *v = (int *)dst + s * E + e; *v = valid ? enc_flat(*v & SYN_CELL, (int)K) : -1; }
                    else if (!valid) ((float *)dst)[s * E + e] = -1.0f;
                }
            return n;
        }
        case HTM_F_SEG_POTENTIAL: {
            if (!c.has_distal) { memset(dst, 0, (size_t)n * 4); return n; }
            int *tmp = nullptr;
            if (hipMalloc((void **)&tmp, (size_t)n * 4) != hipSuccess) { h->err = "htm_read_rows: hipMalloc failed"; return HTM_ERR_HIP; }
            hipLaunchKernelGGL(k_tm_potentials, dim3((unsigned)std::min<int64_t>((n * 8 + 255) / 256, 8192)), dim3(256), 0, h->stream, d, q, tmp,
                               (int)row_begin, (int)(row_begin + row_count));
            const bool ok = hipStreamSynchronize(h->stream) == hipSuccess && hipMemcpy(dst, tmp, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
            hipFree(tmp);
            if (!ok) { h->err = "htm_read_rows: potentials kernel failed"; return HTM_ERR_HIP; }
            return n;
        }
        case HTM_F_MATCH_INFO: {
            const int64_t w0 = row_begin >> 5, w1 = (row_begin + row_count + 31) >> 5;
            std::vector<uint32_t> bits((size_t)(w1 - w0), 0u);
            if (c.has_distal && hipMemcpy(bits.data(), d.match_bits[q] + w0, bits.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) { h->err = "htm_read_rows: hipMemcpy failed"; return HTM_ERR_HIP; }
            if (!copy(d.seg_info + row_begin, (size_t)n * 4)) return HTM_ERR_HIP;
            for (int64_t i = 0; i < n; ++i) {
                const int64_t r = row_begin + i;
                const bool m = (bits[(size_t)((r >> 5) - w0)] >> (r & 31)) & 1u;
                ((uint32_t *)dst)[i] = m ? (((uint32_t *)dst)[i] & ~0x40000000u) : 0u;
            }
            return n;
        }
        default: h->err = "htm_read_rows: not a per-segment field"; return HTM_ERR_ARGUMENT;
    }
}

extern "C" int htm_write(htm_handle *h, int32_t field, const void *src, int64_t count) {
    if (!h || (!src && count > 0) || count < 0) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (field == HTM_F_SEG_CELL || field == HTM_F_SEG_NSYN || field == HTM_F_SEG_PRESYN || field == HTM_F_SEG_PERM || field == HTM_F_SEGCOUNT) {
        REFUSE_ON_VIEW(h, "htm_write of a weight field");
        weights_touched(h);
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    Dev &d = h->d;
    const bool sp = h->cfg.enable_sp, tm = h->cfg.enable_tm;
    const int64_t C = d.C, K = d.K, E = d.E;
    const int q = (int)((h->step_host + 1) & 1);      // becomes "previous step" for the next one
    auto put = [&](void *dstp, const void *s, int64_t n, size_t elem, int64_t cap) -> int {
        if (n > cap) { h->err = "htm_write: too many elements"; return HTM_ERR_ARGUMENT; }
        if (n > 0 && hipMemcpy(dstp, s, (size_t)n * elem, hipMemcpyHostToDevice) != hipSuccess) { h->err = "htm_write: hipMemcpy failed"; return HTM_ERR_HIP; }
        return HTM_OK;
    };
    if (((field >= HTM_F_CELL_ACTIVATION) && !tm) || ((field >= HTM_F_OVERLAPS && field <= HTM_F_DUTY_CYCLE) && !sp)) {
        h->err = "htm_write: field not available on this handle";
        return HTM_ERR_STATE;
    }
    if (h->world > 1 && (field == HTM_F_SEG_CELL || field == HTM_F_SEG_NSYN || field == HTM_F_SEG_PRESYN || field == HTM_F_SEG_PERM)) {
        // a column-sharded handle is given the arrays of ALL segment ids (what an unsharded handle exports, or the merged
        // export of a sharded group) and keeps its own cells' rows at the commit
        const int64_t per = (field == HTM_F_SEG_PRESYN || field == HTM_F_SEG_PERM) ? E : 1;
        if (count > (int64_t)d.Scap * per) { h->err = "htm_write: too many elements"; return HTM_ERR_ARGUMENT; }
        if (field == HTM_F_SEG_PERM) { h->imp_perm.assign((const float *)src, (const float *)src + count); return HTM_OK; }
        std::vector<int> &v = field == HTM_F_SEG_CELL ? h->imp_seg_cell : field == HTM_F_SEG_NSYN ? h->imp_seg_nsyn : h->imp_presyn;
        v.assign((const int *)src, (const int *)src + count);
        if (field != HTM_F_SEG_NSYN) for (auto &x : v) x = x < 0 ? 0 : flat_enc(x, (int)K);
        return HTM_OK;
    }
    switch (field) {
        case HTM_F_DUTY_CYCLE: return put(d.duty, src, count, 4, C);
        case HTM_F_CELL_ACTIVATION: return put(d.act[q], src, count, 4, C * d.WPC);
        case HTM_F_CELL_PREDICTION: return put(d.pred[q], src, count, 4, C * d.WPC);
        case HTM_F_SEG_NSYN: return put(d.seg_nsyn, src, count, 4, d.Scap);
        case HTM_F_SEG_POTENTIAL: h->imp_pot.assign((const int *)src, (const int *)src + count); return HTM_OK;
        case HTM_F_MATCH_SEGMENT: h->imp_match_seg.assign((const int *)src, (const int *)src + count); return HTM_OK;
        case HTM_F_MATCH_INFO: h->imp_match_info.assign((const uint32_t *)src, (const uint32_t *)src + count); return HTM_OK;
        case HTM_F_MATCH_JITTER: h->imp_match_jit.assign((const float *)src, (const float *)src + count); return HTM_OK;
        case HTM_F_SEG_PERM: return put(d.sperm, src, count, 4, (int64_t)d.Scap * E);
        case HTM_F_WINNER_CELL:
        case HTM_F_SEG_CELL:
        case HTM_F_SEG_PRESYN: {
            std::vector<int> v((const int *)src, (const int *)src + count);
            for (auto &x : v) x = x < 0 ? 0 : flat_enc(x, (int)K);
            if (field == HTM_F_WINNER_CELL) return put(d.winners[q], v.data(), count, 4, (int64_t)d.k * d.KP);
            if (field == HTM_F_SEG_CELL) return put(d.seg_cell, v.data(), count, 4, d.Scap);
            return put(d.presyn, v.data(), count, 4, (int64_t)d.Scap * E);
        }
        case HTM_F_SEGCOUNT:
        case HTM_F_CELL_MAX_JITTER: {
            if (count != C * K) { h->err = "htm_write: need column_dim * cell_dim elements"; return HTM_ERR_ARGUMENT; }
            std::vector<uint32_t> tmp((size_t)C * d.KP, 0u);
            const uint32_t *v = (const uint32_t *)src;
            for (int64_t col = 0; col < C; ++col)
                for (int64_t j = 0; j < K; ++j) tmp[(size_t)col * d.KP + j] = v[col * K + j];
            return put(field == HTM_F_SEGCOUNT ? (void *)d.segcount : (void *)d.cellmax[q], tmp.data(), (int64_t)tmp.size(), 4, (int64_t)tmp.size());
        }
        default: h->err = "htm_write: field is not writable"; return HTM_ERR_ARGUMENT;
    }
}

extern "C" int htm_import_begin(htm_handle *h, int64_t step_index) {
    if (!h || (step_index < 0 && step_index != HTM_IMPORT_PREV_STATE)) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (h->world > 1 && step_index == HTM_IMPORT_PREV_STATE) { h->err = "prev_state adoption is not available on a column-sharded handle"; return HTM_ERR_STATE; }
    if (step_index != HTM_IMPORT_PREV_STATE) REFUSE_ON_VIEW(h, "a state import (other than HTM_IMPORT_PREV_STATE)");
    if (h->shard_open) { h->err = "htm_import_begin: a step opened with htm_shard_begin is not finished"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->import_keep = step_index == HTM_IMPORT_PREV_STATE;
    if (!h->import_keep) h->step_host = step_index;
    int rc = close_open_phases(h);
    if (rc) return rc;
    return HTM_OK;
}

// winner words (d.win[q], what HTM_F_WINNER_WORDS and State.winner_cell read) from the imported winner list
__global__ __launch_bounds__(256) void k_tm_winner_words(Dev d, int q, int n) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < d.C * d.WPC; c += gridDim.x * 256) d.win[q][c] = 0;
}
__global__ __launch_bounds__(256) void k_tm_winner_bits(Dev d, int q, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) { const int e = d.winners[q][i]; atomicOr(&d.win[q][e >> 5], 1u << (e & 31)); }
}

extern "C" int htm_import_commit(htm_handle *h, int32_t segments, int32_t matching_segments, int32_t winner_cells,
                                 int32_t has_distal_state, int32_t has_winner_cells) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    Dev &d = h->d;
    const bool keep = h->import_keep;              // TemporalMemory.process(prev_state=X): the previous step's State only
    h->import_keep = false;
    if (!keep) REFUSE_ON_VIEW(h, "a state import (other than HTM_IMPORT_PREV_STATE)");
    if (!keep) weights_touched(h);
    Counters c;
    int rc = read_counters(h, &c);
    if (rc) return rc;
    if (keep) segments = c.S;                       // (the store stays what it is)
    if (segments < 0 || segments > d.Scap || matching_segments < 0 || matching_segments > segments ||
        winner_cells < 0 || winner_cells > d.k * d.KP) { h->err = "htm_import_commit: bad scalars"; return HTM_ERR_ARGUMENT; }
    const int q = (int)((h->step_host + 1) & 1);
    std::vector<int> g2l;                           // column-sharded: local row of every id this rank owns, -1 otherwise
    if (h->world > 1) {
        const size_t S = (size_t)segments, E = (size_t)d.E;
        if (h->imp_seg_cell.size() != S || h->imp_seg_nsyn.size() != S || h->imp_presyn.size() != S * E || h->imp_perm.size() != S * E) {
            h->err = "htm_import_commit: a column-sharded handle needs SEG_CELL / SEG_NSYN / SEG_PRESYN / SEG_PERM of all segment ids";
            return HTM_ERR_ARGUMENT;
        }
        g2l.assign((size_t)d.Scap, -1);
        std::vector<int> gid_of_row;
        std::vector<uint32_t> dead(((size_t)d.Scap + 31) / 32 + 32, 0u);
        const size_t nb1 = ((size_t)d.Scap + 1023) / 1024, nb2 = (nb1 + 1023) / 1024 + 1;
        std::vector<int> cnt1(nb1, 0), cnt2(nb2, 0);
        for (size_t g = 0; g < S; ++g) {
            if (h->imp_seg_nsyn[g] < d.match_thr) { dead[g >> 5] |= 1u << (g & 31); cnt1[g >> 10] += 1; cnt2[g >> 20] += 1; }
            const int col = h->imp_seg_cell[g] >> 5;
            if (col >= d.c0 && col < d.c1) { g2l[g] = (int)gid_of_row.size(); gid_of_row.push_back((int)g); }
        }
        const size_t L = gid_of_row.size();
        if (L > (size_t)d.Lcap) { h->err = "htm_import_commit: more segments of this rank's cells than segment_capacity_local"; return HTM_ERR_CAPACITY; }
        std::vector<int> cell(L), nsyn(L), presyn(L * E);
        std::vector<float> perm(L * E);
        for (size_t r = 0; r < L; ++r) {
            const size_t g = (size_t)gid_of_row[r];
            cell[r] = h->imp_seg_cell[g];
            nsyn[r] = h->imp_seg_nsyn[g];
            memcpy(&presyn[r * E], &h->imp_presyn[g * E], E * 4);
            memcpy(&perm[r * E], &h->imp_perm[g * E], E * 4);
        }
        HIPCHK(h, hipMemset(d.seg_gid, 0xFF, (size_t)d.Lcap * 4));
        HIPCHK(h, hipMemset(d.seg_nsyn, 0, (size_t)d.Lcap * 4));
        if (L) {
            HIPCHK(h, hipMemcpy(d.seg_gid, gid_of_row.data(), L * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d.seg_cell, cell.data(), L * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d.seg_nsyn, nsyn.data(), L * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d.presyn, presyn.data(), L * E * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d.sperm, perm.data(), L * E * 4, hipMemcpyHostToDevice));
        }
        HIPCHK(h, hipMemcpy(d.g2l, g2l.data(), g2l.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d.dead_bits, dead.data(), dead.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d.recyc_cnt, cnt1.data(), cnt1.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(d.recyc_cnt2, cnt2.data(), cnt2.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemset(d.dead_list, 0, sizeof(int)));
        c.L = (int32_t)L;
        c.n_lfree = 0;
        h->imp_seg_cell.clear(); h->imp_seg_nsyn.clear(); h->imp_presyn.clear(); h->imp_perm.clear();
        h->imp_seg_cell.shrink_to_fit(); h->imp_presyn.shrink_to_fit(); h->imp_perm.shrink_to_fit();
    }
    const int rows = h->world > 1 ? c.L : segments;     // rows of the per-row arrays (info words, jitter, match bits)
    auto row_of = [&](int gid) { return h->world > 1 ? g2l[(size_t)gid] : gid; };
    if (!keep) {
        c.step[h->step_host & 1] = (uint32_t)h->step_host;
        c.n_work[0] = c.n_work[1] = 0;
        c.n_bind[0] = c.n_bind[1] = 0;
        c.S = segments;
        h->seg_hint = rows;                         // (the one place where the count can go down)
        if (h->seg_pinned) *h->seg_pinned = rows;
    }
    {   // dense per-segment info from the staged PredictiveProjection.State lists
        const size_t M = (size_t)matching_segments;
        if (has_distal_state && (h->imp_pot.size() != (size_t)segments || h->imp_match_seg.size() != M ||
                                 h->imp_match_info.size() != M || h->imp_match_jit.size() != M)) {
            h->err = "htm_import_commit: SEG_POTENTIAL / MATCH_* fields missing or of the wrong length";
            return HTM_ERR_ARGUMENT;
        }
        std::vector<uint32_t> info((size_t)rows, 0u), bits((size_t)(d.Lcap + 255) / 256 * 8, 0u);
        std::vector<float> jit((size_t)rows, 0.f);
        if (has_distal_state) {
            for (size_t i = 0; i < M; ++i) {
                if (h->imp_match_seg[i] < 0 || h->imp_match_seg[i] >= segments) { h->err = "htm_import_commit: matching segment id out of range"; return HTM_ERR_ARGUMENT; }
                const int sgm = row_of(h->imp_match_seg[i]);
                if (sgm < 0) continue;              // (another rank's segment)
                info[(size_t)sgm] = (h->imp_match_info[i] & ~0x40000000u) | 0x40000000u;
                jit[(size_t)sgm] = h->imp_match_jit[i];
                bits[(size_t)sgm >> 5] |= 1u << (sgm & 31);
            }
        }
        if (rows) {
            HIPCHK(h, hipMemcpy(d.seg_info, info.data(), info.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(d.seg_jit, jit.data(), jit.size() * 4, hipMemcpyHostToDevice));
        }
        // all of the bitmap: the import is the one place where the segment count can shrink (rollback to an
        // earlier checkpoint), and ids at or above it must read "not matching", as the classification assumes
        HIPCHK(h, hipMemcpy(d.match_bits[q], bits.data(), bits.size() * 4, hipMemcpyHostToDevice));
        // the other buffers (what the coming step's scan accumulates into) start clean
        HIPCHK(h, hipMemset(d.match_bits[q ^ 1], 0, bits.size() * 4));
        HIPCHK(h, hipMemset(d.cellmax[q ^ 1], 0, (size_t)d.C * d.KP * 4));
        h->imp_pot.clear(); h->imp_match_seg.clear(); h->imp_match_info.clear(); h->imp_match_jit.clear();
    }
    c.n_win[q] = winner_cells;
    c.has_winner[q] = has_winner_cells ? 1 : 0;
    c.has_distal = has_distal_state ? 1 : 0;
    c.cm_dense_step = (uint32_t)h->step_host + 1u;
    if (!keep) h->window_known = false;
    if (!keep) c.error = 0;                         // a checkpoint restore starts clean; an adopted previous State does not
                                                    // forgive an overflow of the store it keeps
    HIPCHK(h, hipMemcpy(d.ctr, &c, sizeof(c), hipMemcpyHostToDevice));
    if (h->cfg.enable_tm) {
        // the previous step's active columns (State.active_cell / winner_cell index with them): the columns with an active cell
        {
            std::vector<uint32_t> act((size_t)d.C * d.WPC);
            HIPCHK(h, hipMemcpy(act.data(), d.act[q], act.size() * 4, hipMemcpyDeviceToHost));
            std::vector<int> cols((size_t)d.k, 0);
            int n = 0;
            for (int col = 0; col < d.C && n < d.k; ++col)
                if (act[(size_t)col * d.WPC] | act[(size_t)col * d.WPC + d.WPC - 1]) cols[(size_t)n++] = col;
            HIPCHK(h, hipMemcpy(d.active_cols[q], cols.data(), cols.size() * 4, hipMemcpyHostToDevice));
        }
        // State.winner_cell / HTM_F_WINNER_WORDS read the winner words: rebuild them from the imported list
        hipLaunchKernelGGL(k_tm_winner_words, dim3(std::min((d.C + 255) / 256, 1024)), dim3(256), 0, h->stream, d, q, winner_cells);
        if (winner_cells > 0) hipLaunchKernelGGL(k_tm_winner_bits, dim3((winner_cells + 255) / 256), dim3(256), 0, h->stream, d, q, winner_cells);
        if (!keep) {
            if (h->world == 1) {                    // (a shard's counts came with its dead bits, above)
                HIPCHK(h, hipMemsetAsync(d.recyc_cnt2, 0, ((size_t)(h->sz.s1024_blocks + 1023) / 1024 + 1) * sizeof(int), h->stream));
                hipLaunchKernelGGL(k_tm_recount, dim3(h->sz.s1024_blocks), dim3(256), 0, h->stream, d);
            }
            hipLaunchKernelGGL(k_tm_flag_connected, dim3(std::min(4096, std::max(1, (int)(((long long)rows * d.E + 255) / 256)))), dim3(256), 0, h->stream, d);
        }
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return HTM_OK;
}

// A sequence reset on the device (htm_reset.h): after the held-back tail, one launch, no host copy, no wait.
extern "C" int htm_reset(htm_handle *h) {
    if (!h) return HTM_ERR_ARGUMENT;
    flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    if (h->world > 1) { h->err = "htm_reset: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    if (h->shard_open) { h->err = "htm_reset: a step opened with htm_shard_begin is not finished"; return HTM_ERR_STATE; }
    if (!h->cfg.enable_tm) { h->err = "htm_reset: the handle has no Temporal Memory"; return HTM_ERR_STATE; }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = view_enter(h, 0);
    if (rc) return rc;
    rc = close_open_phases(h);
    if (rc) return rc;
    LAUNCH(h, "tm_reset", k_tm_reset, reset_blocks(h->d), 256, h->d, (int)(h->step_host & 1), (const ResetDev *)nullptr, (RecDev *)nullptr,
           (uint32_t)h->step_host);
    return launch_status(h->err);
}

extern "C" int htm_set_run_resets(htm_handle *h, const uint32_t *device_bits, int32_t n_inputs) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (device_bits && n_inputs < 1) { h->err = "htm_set_run_resets: n_inputs must be at least 1"; return HTM_ERR_ARGUMENT; }
    if (h->world > 1) { h->err = "htm_set_run_resets: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    h->reset_bits = device_bits;
    h->reset_n = device_bits ? n_inputs : 0;
    return HTM_OK;
}

// Predicted-input decoding (htm_decode.h): a handle whose Spatial Pooler and Temporal Memory are both the device's own
static int pin_refuse(htm_handle *h, const char *what) {
    if (h->world > 1) { h->err = std::string(what) + ": not available on a column-sharded handle"; return HTM_ERR_STATE; }
    if (!h->cfg.enable_sp || !h->cfg.enable_tm) { h->err = std::string(what) + ": needs a handle with the device's own Spatial Pooler and Temporal Memory"; return HTM_ERR_STATE; }
    return 0;
}

extern "C" int htm_set_run_predicted_input(htm_handle *h, int32_t *device_votes) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (device_votes) { int rc = pin_refuse(h, "htm_set_run_predicted_input"); if (rc) return rc; }
    h->pin_out = device_votes;
    return HTM_OK;
}

// Pattern capture (htm_classifier.h, kcls_capture): the rows go into the device descriptor here, on the handle's stream, from the
// call's own word (read when the copy returns) -- the runs that follow, and the graphs they replay, read them through it
extern "C" int htm_set_run_active_cells(htm_handle *h, void *device_pairs) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!device_pairs) { h->cap_out = nullptr; return HTM_OK; }
    if (int rc = pin_refuse(h, "htm_set_run_active_cells")) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_cap) { if (int rc = dalloc(h, &h->d_cap, 1)) return rc; }
    const ClsCapDev cap{(ClsPair *)device_pairs};
    HIPCHK(h, hipMemcpyAsync(h->d_cap, &cap, sizeof(cap), hipMemcpyHostToDevice, h->stream));
    h->cap_out = device_pairs;
    return HTM_OK;
}

// After the held-back tail: the output row zeroed, one launch, a synchronising copy (as htm_read)
extern "C" int htm_predicted_input(htm_handle *h, int32_t *host_dst) {
    if (!h || !host_dst) return HTM_ERR_ARGUMENT;
    flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    int rc = pin_refuse(h, "htm_predicted_input");
    if (rc) return rc;
    if (h->shard_open || h->phase_open) { h->err = "htm_predicted_input: a step of the handle is open (htm_shard_begin / htm_sp_phase)"; return HTM_ERR_STATE; }
    rc = view_enter(h, 0);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const Dev &d = h->d;
    if (!h->d_pin_buf) { rc = dalloc(h, &h->d_pin_buf, d.I); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->d_pin_buf, 0, (size_t)d.I * 4, h->stream));
    LAUNCH(h, "predicted_input", k_pin, pin_blocks(d.C), 256, d, (int)((h->step_host + 1) & 1), h->d_pin_buf);
    rc = launch_status(h->err);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(host_dst, h->d_pin_buf, (size_t)d.I * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

// Closed-loop forecasting (htm_forecast.h).  The scratch votes row and the descriptor, allocated when first needed.
static int feed_alloc(htm_handle *h) {
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->d_feed_votes) { int rc = dalloc(h, &h->d_feed_votes, h->d.I); if (rc) return rc; }      // (zeroed: dalloc)
    if (!h->d_feed) { int rc = dalloc(h, &h->d_feed, 1); if (rc) return rc; }
    return 0;
}

static int feed_check_args(htm_handle *h, const char *what, int32_t min_votes, int32_t max_bits, const uint32_t *bank, int32_t rows) {
    if (min_votes < 1 || max_bits < 0 || rows < 1) { h->err = std::string(what) + ": min_votes >= 1, max_bits >= 0 and at least one bank row"; return HTM_ERR_ARGUMENT; }
    if (((uintptr_t)bank & 15) != 0) { h->err = std::string(what) + ": the bank must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    return 0;
}

// After the held-back tail: the votes of the current state into the scratch row, then the row encoded; no copy, no wait
extern "C" int htm_encode_votes(htm_handle *h, int32_t min_votes, int32_t max_bits, uint32_t *device_bank, int32_t bank_rows, int32_t row) {
    if (!h || !device_bank) return HTM_ERR_ARGUMENT;
    flush_tail(h);
    int rc = feed_check_args(h, "htm_encode_votes", min_votes, max_bits, device_bank, bank_rows);
    if (rc) return rc;
    if (row < 0 || row >= bank_rows) { h->err = "htm_encode_votes: 0 <= row < bank_rows"; return HTM_ERR_ARGUMENT; }
    REJECT_WHEN_AHEAD(h);
    rc = pin_refuse(h, "htm_encode_votes");
    if (rc) return rc;
    if (h->shard_open || h->phase_open) { h->err = "htm_encode_votes: a step of the handle is open (htm_shard_begin / htm_sp_phase)"; return HTM_ERR_STATE; }
    rc = view_enter(h, 0);
    if (rc) return rc;
    rc = feed_alloc(h);
    if (rc) return rc;
    const Dev &d = h->d;
    LAUNCH(h, "feedback_votes", k_pin, pin_blocks(d.C), 256, d, (int)((h->step_host + 1) & 1), h->d_feed_votes);
    LAUNCH(h, "feedback_encode", k_encode, 1, ENC_THREADS, d, h->d_feed_votes, (int)min_votes, (int)max_bits, device_bank + (size_t)row * d.W);
    return launch_status(h->err);
}

extern "C" int htm_set_run_feedback(htm_handle *h, uint32_t *device_bank, int32_t n_inputs, int32_t min_votes, int32_t max_bits) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!device_bank) {                             // cleared: the descriptor too (group launches read it)
        h->feed_bank = nullptr;
        h->feed_n = 0;
        if (h->d_feed) {
            HIPCHK(h, hipSetDevice(h->device));
            LAUNCH(h, "feedback_set", k_feed_set, 1, 64, h->d_feed, (uint32_t *)nullptr, h->d_feed_votes, 0, 1, 0);
            return launch_status(h->err);
        }
        return HTM_OK;
    }
    int rc = pin_refuse(h, "htm_set_run_feedback");
    if (rc) return rc;
    rc = feed_check_args(h, "htm_set_run_feedback", min_votes, max_bits, device_bank, n_inputs);
    if (rc) return rc;
    REJECT_WHEN_AHEAD(h);
    rc = feed_alloc(h);
    if (rc) return rc;
    LAUNCH(h, "feedback_set", k_feed_set, 1, 64, h->d_feed, device_bank, h->d_feed_votes, n_inputs, min_votes, max_bits);
    rc = launch_status(h->err);
    if (rc) return rc;
    h->feed_bank = device_bank;
    h->feed_n = n_inputs;
    return HTM_OK;
}

// Region stacks (htm_stack.h): bank rows for h from the active-column lists a lower region's recorded run left on the device
extern "C" int htm_pack_columns(htm_handle *h, const int32_t *device_lists, int32_t k, int32_t n_rows, int32_t stride,
                                uint32_t *device_bank, int32_t bank_rows, int32_t first_row) {
    if (!h || !device_lists || !device_bank) return HTM_ERR_ARGUMENT;
    if (k < 1 || stride < 1 || n_rows < 0 || bank_rows < 1 || first_row < 0 || first_row >= bank_rows) {
        h->err = "htm_pack_columns: k >= 1, stride >= 1, n_rows >= 0, bank_rows >= 1 and 0 <= first_row < bank_rows";
        return HTM_ERR_ARGUMENT;
    }
    if (((uintptr_t)device_bank & 15) != 0) { h->err = "htm_pack_columns: the bank must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    if (!h->cfg.enable_sp) { h->err = "htm_pack_columns: needs a handle with the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_pack_columns: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REJECT_WHEN_AHEAD(h);
    if (pack_lds(h->d) > PACK_LDS_MAX) { h->err = "htm_pack_columns: an input row of this handle does not fit the LDS (input_dim above 524288)"; return HTM_ERR_ARGUMENT; }
    if (n_rows == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    LAUNCH_ON(h, h->stream, pack_lds(h->d), "pack_columns", k_pack_columns, n_rows, PACK_THREADS, h->d, device_lists, k, stride, device_bank,
              bank_rows, first_row);
    return launch_status(h->err);
}

// Pooling links (htm_pool.h): bank rows for h from the lists and the column predictions a lower region's recorded run left on the
// device, through the link's state arrays; per batch of the windows that fit the caller's scratch, the pack launch at stride 1,
// the scan and the select
extern "C" int htm_pool_columns(htm_handle *h, htm_pool_link link, const int32_t *device_lists, int32_t k, const uint32_t *device_column_prediction,
                                int32_t n_rows, uint8_t *device_persistence, uint32_t *device_prev, const uint32_t *device_reset_bits,
                                void *device_scratch, int64_t scratch_bytes, uint32_t *device_bank, int32_t bank_rows, int32_t first_row) {
    if (!h || !device_lists || !device_bank) return HTM_ERR_ARGUMENT;
    if (!device_column_prediction || !device_persistence || !device_prev || !device_scratch) {
        h->err = "htm_pool_columns: null column prediction, state or scratch";
        return HTM_ERR_ARGUMENT;
    }
    if (link.struct_bytes != sizeof(htm_pool_link)) { h->err = "htm_pool_columns: struct_bytes != sizeof(htm_pool_link)"; return HTM_ERR_ARGUMENT; }
    if (k < 1 || link.stride < 1 || n_rows < 0 || bank_rows < 1 || first_row < 0 || first_row >= bank_rows) {
        h->err = "htm_pool_columns: k >= 1, stride >= 1, n_rows >= 0, bank_rows >= 1 and 0 <= first_row < bank_rows";
        return HTM_ERR_ARGUMENT;
    }
    if (link.active_weight < 0 || link.active_weight > 255 || link.predicted_weight < 0 || link.predicted_weight > 255 ||
        (link.active_weight == 0 && link.predicted_weight == 0)) {
        h->err = "htm_pool_columns: 0 <= active_weight, predicted_weight <= 255, not both 0";
        return HTM_ERR_ARGUMENT;
    }
    if (link.decay < 1 || link.decay > 255 || link.ceiling < 1 || link.ceiling > 255) {
        h->err = "htm_pool_columns: 1 <= decay <= 255 and 1 <= ceiling <= 255";
        return HTM_ERR_ARGUMENT;
    }
    if (((uintptr_t)device_bank & 15) != 0) { h->err = "htm_pool_columns: the bank must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    if ((((uintptr_t)device_persistence | (uintptr_t)device_prev | (uintptr_t)device_scratch) & 15) != 0) {
        h->err = "htm_pool_columns: the persistence, the prev words and the scratch must be 16-byte aligned";
        return HTM_ERR_ARGUMENT;
    }
    if (!h->cfg.enable_sp) { h->err = "htm_pool_columns: needs a handle with the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
    if (h->world > 1) { h->err = "htm_pool_columns: not available on a column-sharded handle"; return HTM_ERR_STATE; }
    REJECT_WHEN_AHEAD(h);
    const int C = h->d.I, W = h->d.W;
    if (C > POOL_MAX_COLUMNS) { h->err = "htm_pool_columns: more lower columns (the handle's input_dim) than HTM_POOL_MAX_COLUMNS (262144)"; return HTM_ERR_ARGUMENT; }
    if (link.union_bits < 1 || link.union_bits > C) { h->err = "htm_pool_columns: 1 <= union_bits <= the handle's input_dim"; return HTM_ERR_ARGUMENT; }
    const size_t window = pool_window_bytes(W, link.stride);
    if (scratch_bytes < 0 || (uint64_t)scratch_bytes < (uint64_t)window) {
        h->err = "htm_pool_columns: the scratch is too small for one window (" + std::to_string(window) + " bytes)";
        return HTM_ERR_ARGUMENT;
    }
    if (n_rows == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    // (a batch's steps are the pack launch's grid: 32-bit)
    const int per_batch = (int)std::min<uint64_t>(std::min<uint64_t>((uint64_t)n_rows, (uint64_t)scratch_bytes / window), (uint64_t)(INT32_MAX / link.stride));
    const int PW = (C + 31) / 32;
    for (long long r0 = 0; r0 < n_rows; r0 += per_batch) {
        const int n = (int)std::min<long long>(per_batch, n_rows - r0);
        const size_t steps = (size_t)n * (size_t)link.stride, first_step = (size_t)r0 * (size_t)link.stride;
        uint32_t *bitmaps = (uint32_t *)device_scratch;
        PoolDev a;
        a.C = C; a.W = W; a.PW = PW;
        a.stride = link.stride; a.n_windows = n;
        a.active_weight = link.active_weight; a.predicted_weight = link.predicted_weight; a.decay = link.decay; a.ceiling = link.ceiling;
        a.union_bits = link.union_bits;
        a.bank_rows = bank_rows; a.first_row = (int)(((long long)first_row + r0) % bank_rows);
        a.bitmaps = bitmaps;
        a.colpred = device_column_prediction + first_step * (size_t)PW;
        a.resets = device_reset_bits;
        a.persistence = device_persistence; a.prev = device_prev;
        a.snap = (uint8_t *)device_scratch + steps * (size_t)W * 4;           // (a multiple of 16 bytes: W is a multiple of 4)
        a.bank = device_bank;
        // the bitmap rows: one per step, row s of the scratch (bank_rows = the batch's steps, no rotation)
        LAUNCH_ON(h, h->stream, pack_lds(h->d), "pool_pack", k_pack_columns, (int)steps, PACK_THREADS, h->d, device_lists + first_step * (size_t)k, k, 1, bitmaps,
                  (int)steps, 0);
        LAUNCH(h, "pool_scan", kpool_scan, (W * 32 + POOL_THREADS - 1) / POOL_THREADS, POOL_THREADS, a);
        LAUNCH_ON(h, h->stream, pool_select_lds(W), "pool_select", kpool_select, n, POOL_THREADS, a);
    }
    return launch_status(h->err);
}

// Device-side input noise (htm_noise.h): ring rows for the steps first_step .. first_step + n_rows - 1 from the rows of a source
// bank and the keyed flips of those steps, and the ring's reset bits from the source's.  Behind whatever the stream holds -- the
// held-back tail of htm_step reads no bank, and a Spatial Pooler that is ahead (HTM_RUN_CONTINUE) has read the row of the coming
// step, which a refill writes again with the words it has
extern "C" int htm_bank_noise(htm_handle *h, const uint32_t *src_bank, int32_t n_src, uint32_t *dst_bank, int32_t n_dst, uint32_t first_step,
                              int32_t n_rows, uint32_t seed, uint32_t threshold24, const uint32_t *src_resets, uint32_t *dst_resets) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!src_bank || !dst_bank) { h->err = "htm_bank_noise: null bank"; return HTM_ERR_ARGUMENT; }
    if (src_bank == dst_bank) { h->err = "htm_bank_noise: the source bank and the destination bank must differ"; return HTM_ERR_ARGUMENT; }
    if (n_src < 1 || n_dst < 1 || n_rows < 0 || n_rows > n_dst) { h->err = "htm_bank_noise: n_src >= 1, n_dst >= 1 and 0 <= n_rows <= n_dst"; return HTM_ERR_ARGUMENT; }
    if (threshold24 > (1u << 24)) { h->err = "htm_bank_noise: threshold24 above 2^24"; return HTM_ERR_ARGUMENT; }
    if ((src_resets == nullptr) != (dst_resets == nullptr)) { h->err = "htm_bank_noise: both reset pointers, or neither"; return HTM_ERR_ARGUMENT; }
    if ((((uintptr_t)src_bank | (uintptr_t)dst_bank) & 15) != 0) { h->err = "htm_bank_noise: the banks must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    if (!h->cfg.enable_sp) { h->err = "htm_bank_noise: needs a handle with the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
    const int blocks = n_rows + (dst_resets ? noise_reset_blocks(n_dst) : 0);
    if (blocks == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    LAUNCH(h, "bank_noise", k_bank_noise, blocks, NOISE_THREADS, h->d, src_bank, n_src, dst_bank, n_dst, first_step, n_rows, seed, threshold24,
           src_resets, dst_resets);
    return launch_status(h->err);
}

// Scalar streams (htm_scalar.h).  The field table of a call, checked -- every field as the definition has it, inside the input
// row, no two overlapping, and for a decoding call no field above the LDS cap -- and copied into the kernel argument
static int scalar_table(htm_handle *h, const char *what, const htm_scalar_field *fields, int32_t n_fields, bool decoding, ScalarTab *tab) {
    const std::string who = what;
    if (!fields) { h->err = who + ": null field table"; return HTM_ERR_ARGUMENT; }
    if (n_fields < 1 || n_fields > HTM_SCALAR_MAX_FIELDS) { h->err = who + ": n_fields outside [1, " + std::to_string(HTM_SCALAR_MAX_FIELDS) + "]"; return HTM_ERR_ARGUMENT; }
    if (!h->cfg.enable_sp) { h->err = who + ": needs a handle with the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
    memset(tab, 0, sizeof(*tab));
    for (int j = 0; j < n_fields; ++j) {
        const htm_scalar_field &f = fields[j];
        const std::string fj = who + ": field " + std::to_string(j);
        // the kind (htm_fields.h): reserved == 0 is a linear field, as every call before the kinds existed passed it
        if (f.reserved < 0) { h->err = fj + ": reserved must be 0, or a field kind (1 category, 2 hashed, 3 coordinate) with a hashed or coordinate field's seed above it"; return HTM_ERR_ARGUMENT; }
        const int kind = f.reserved & 3;
        if (kind != HTM_FIELD_LINEAR && f.periodic != 0) { h->err = fj + ": only a linear field can be periodic"; return HTM_ERR_ARGUMENT; }
        if (kind == HTM_FIELD_COORDINATE && f.bits == 0) {
            // a continuation of a coordinate group (htm_coord.h): the y or the radius column, right behind its head; it holds no bits
            const int head = j >= 1 && coord_head(fields[j - 1]) ? j - 1 : j >= 2 && coord_head(fields[j - 2]) && coord_tail(fields[j - 1]) ? j - 2 : -1;
            if (head < 0) { h->err = fj + ": a coordinate continuation (kind 3, bits 0) that is not the first or second entry behind a head"; return HTM_ERR_ARGUMENT; }
            if (f.reserved != HTM_FIELD_COORDINATE || f.width != 0 || f.buckets != 0 || f.offset != fields[head].offset) {
                h->err = fj + ": a coordinate continuation takes reserved 3, width 0, buckets 0 and its head's offset";
                return HTM_ERR_ARGUMENT;
            }
            if (!std::isfinite(f.minimum) || !std::isfinite(f.scale) || !(f.scale > 0.0)) { h->err = fj + ": minimum and scale must be finite, scale above 0"; return HTM_ERR_ARGUMENT; }
            tab->f[j] = f;
            continue;
        }
        if (kind != HTM_FIELD_HASHED && kind != HTM_FIELD_COORDINATE && (f.reserved >> 2) != 0) { h->err = fj + ": a seed on a field that is neither hashed nor a coordinate head"; return HTM_ERR_ARGUMENT; }
        if (f.bits < 1 || f.width < 1) { h->err = fj + ": bits >= 1 and width >= 1"; return HTM_ERR_ARGUMENT; }
        if (kind == HTM_FIELD_LINEAR) {
            if (f.width > f.bits) { h->err = fj + ": bits >= 1 and 1 <= width <= bits"; return HTM_ERR_ARGUMENT; }
            if (f.buckets != (f.periodic ? f.bits : f.bits - f.width + 1)) { h->err = fj + ": buckets must be bits (periodic) or bits - width + 1"; return HTM_ERR_ARGUMENT; }
        } else if (kind == HTM_FIELD_CATEGORY) {
            if (f.buckets < 1 || (long long)f.buckets * f.width > (long long)f.bits) { h->err = fj + ": a category field needs buckets >= 1 and buckets * width <= bits"; return HTM_ERR_ARGUMENT; }
        } else if (kind == HTM_FIELD_COORDINATE) {
            if (f.width > HTM_HASHED_MAX_WIDTH || f.buckets < 0 || f.buckets > HTM_COORD_MAX_RADIUS) {
                h->err = fj + ": a coordinate field needs width <= " + std::to_string(HTM_HASHED_MAX_WIDTH) + " and max_radius (buckets) in [0, " + std::to_string(HTM_COORD_MAX_RADIUS) + "]";
                return HTM_ERR_ARGUMENT;
            }
            if (j + 2 >= n_fields || !coord_tail(fields[j + 1]) || !coord_tail(fields[j + 2])) {
                h->err = fj + ": a coordinate head (kind 3, bits >= 1) must be followed by its two continuations (kind 3, bits 0): the y and the radius column";
                return HTM_ERR_ARGUMENT;
            }
        } else {
            if (f.buckets < 1 || f.width > HTM_HASHED_MAX_WIDTH || f.buckets > INT32_MAX - HTM_HASHED_MAX_WIDTH) {
                h->err = fj + ": a hashed field needs buckets >= 1 (below 2^31 - " + std::to_string(HTM_HASHED_MAX_WIDTH) + ") and width <= " + std::to_string(HTM_HASHED_MAX_WIDTH);
                return HTM_ERR_ARGUMENT;
            }
            if (decoding && (long long)f.buckets + f.width - 1 > HTM_DECODE_MAX_BITS) {
                h->err = fj + ": buckets + width - 1 above " + std::to_string(HTM_DECODE_MAX_BITS) + " (the decode launch's LDS)";
                return HTM_ERR_ARGUMENT;
            }
        }
        if (f.offset < 0 || (long long)f.offset + f.bits > (long long)h->d.I) { h->err = fj + ": reaches outside the input row"; return HTM_ERR_ARGUMENT; }
        if (!std::isfinite(f.minimum) || !std::isfinite(f.scale) || !(f.scale > 0.0)) { h->err = fj + ": minimum and scale must be finite, scale above 0"; return HTM_ERR_ARGUMENT; }
        if (decoding && kind != HTM_FIELD_HASHED && kind != HTM_FIELD_COORDINATE && f.bits > HTM_DECODE_MAX_BITS) { h->err = fj + ": more than " + std::to_string(HTM_DECODE_MAX_BITS) + " bits (the decode launch's LDS)"; return HTM_ERR_ARGUMENT; }
        for (int i = 0; i < j; ++i)                 // (a continuation has no bits: it overlaps nothing)
            if (fields[i].bits > 0 && f.offset < fields[i].offset + fields[i].bits && fields[i].offset < f.offset + f.bits) { h->err = fj + ": overlaps field " + std::to_string(i); return HTM_ERR_ARGUMENT; }
        tab->f[j] = f;
        tab->f[j].periodic = f.periodic != 0;       // (reserved stays: the kind and the seed, 0 for a linear field)
    }
    return 0;
}

// The kernels of a checked table: those of htm_coord.h where it holds a coordinate field, else the twins of htm_fields.h where it
// holds a category or hashed field, else the linear kernels of htm_scalar.h and htm_live.h.  kcoord_bank's block is SCALAR_THREADS
// threads whatever the row's width (its select wants them); the others' follow the row
enum FieldPath { FIELDS_LINEAR, FIELDS_MIXED, FIELDS_COORDINATE };
static FieldPath field_path(const ScalarTab &tab, int n_fields) {
    return fields_coordinate(tab.f, n_fields) ? FIELDS_COORDINATE : fields_mixed(tab.f, n_fields) ? FIELDS_MIXED : FIELDS_LINEAR;
}
static decltype(&k_bank_encode) encode_kernel(FieldPath p) { return p == FIELDS_COORDINATE ? kcoord_bank : p == FIELDS_MIXED ? kenc_bank : k_bank_encode; }
static int encode_threads(FieldPath p, int W) { return p == FIELDS_COORDINATE ? SCALAR_THREADS : scalar_encode_threads(W); }
static decltype(&k_decode_votes) votes_kernel(FieldPath p) { return p == FIELDS_COORDINATE ? kcoord_votes : p == FIELDS_MIXED ? kenc_votes : k_decode_votes; }
static decltype(&klive_finish) finish_kernel(FieldPath p) { return p == FIELDS_COORDINATE ? kcoord_finish : p == FIELDS_MIXED ? kenc_finish : klive_finish; }

// Bank rows from values: one launch behind whatever the stream holds, no copy, no wait, no state of the handle read (as
// htm_bank_noise: also on a view, also while the handle is ahead)
extern "C" int htm_bank_encode(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, const double *device_values, int32_t n_rows,
                               uint32_t *device_bank, int32_t bank_rows, int32_t first_row) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!device_values || !device_bank) { h->err = "htm_bank_encode: null values or bank"; return HTM_ERR_ARGUMENT; }
    ScalarTab tab;
    int rc = scalar_table(h, "htm_bank_encode", fields, n_fields, false, &tab);
    if (rc) return rc;
    if (n_rows < 0 || first_row < 0 || (long long)first_row + n_rows > (long long)bank_rows) {
        h->err = "htm_bank_encode: n_rows >= 0, first_row >= 0 and first_row + n_rows <= bank_rows";
        return HTM_ERR_ARGUMENT;
    }
    if (((uintptr_t)device_bank & 15) != 0 || ((uintptr_t)device_values & 7) != 0) { h->err = "htm_bank_encode: the bank must be 16-byte aligned, the values 8-byte"; return HTM_ERR_ARGUMENT; }
    if (n_rows == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    const FieldPath path = field_path(tab, n_fields);
    LAUNCH(h, "bank_encode", encode_kernel(path), n_rows, encode_threads(path, h->d.W), h->d, tab, (int)n_fields, device_values, device_bank, (int)first_row);
    return launch_status(h->err);
}

// A bucket and a score per row and field from rows of votes: one launch, no copy, no wait, no state of the handle read
extern "C" int htm_decode_votes(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, const int32_t *device_votes, int32_t n_rows,
                                int32_t *device_out) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!device_votes || !device_out) { h->err = "htm_decode_votes: null votes or output"; return HTM_ERR_ARGUMENT; }
    ScalarTab tab;
    int rc = scalar_table(h, "htm_decode_votes", fields, n_fields, true, &tab);
    if (rc) return rc;
    if (n_rows < 0) { h->err = "htm_decode_votes: n_rows must not be negative"; return HTM_ERR_ARGUMENT; }
    if (n_rows == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(h->device));
    LAUNCH(h, "decode_votes", votes_kernel(field_path(tab, n_fields)), dim3(n_rows, n_fields), SCALAR_THREADS, tab, (int)n_fields, h->d.I, device_votes, device_out);
    return launch_status(h->err);
}

// htm_predicted_input with the votes kept on the device: the votes row zeroed, the votes launch, the decode launch, and one
// synchronising copy of 2 x n_fields ints
extern "C" int htm_predicted_value(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, int32_t *host_out) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (!host_out) { h->err = "htm_predicted_value: null output"; return HTM_ERR_ARGUMENT; }
    ScalarTab tab;
    int rc = scalar_table(h, "htm_predicted_value", fields, n_fields, true, &tab);
    if (rc) return rc;
    flush_tail(h);
    REJECT_WHEN_AHEAD(h);
    rc = pin_refuse(h, "htm_predicted_value");
    if (rc) return rc;
    if (h->shard_open || h->phase_open) { h->err = "htm_predicted_value: a step of the handle is open (htm_shard_begin / htm_sp_phase)"; return HTM_ERR_STATE; }
    rc = view_enter(h, 0);
    if (rc) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const Dev &d = h->d;
    if (!h->d_pin_buf) { rc = dalloc(h, &h->d_pin_buf, d.I); if (rc) return rc; }
    if (!h->d_value_out) { rc = dalloc(h, &h->d_value_out, 2 * HTM_SCALAR_MAX_FIELDS); if (rc) return rc; }
    HIPCHK(h, hipMemsetAsync(h->d_pin_buf, 0, (size_t)d.I * 4, h->stream));
    LAUNCH(h, "predicted_input", k_pin, pin_blocks(d.C), 256, d, (int)((h->step_host + 1) & 1), h->d_pin_buf);
    LAUNCH(h, "decode_votes", votes_kernel(field_path(tab, n_fields)), dim3(1, n_fields), SCALAR_THREADS, tab, (int)n_fields, d.I, (const int32_t *)h->d_pin_buf, h->d_value_out);
    rc = launch_status(h->err);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(host_out, h->d_value_out, (size_t)n_fields * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

extern "C" int htm_profile(htm_handle *h, int32_t enable) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    h->profile = enable != 0;
    return HTM_OK;
}

extern "C" int64_t htm_trace_read(htm_handle *h, uint64_t *dst, int64_t count) {
    if (!h || !dst) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    if (!h->d.trace) { h->err = "htm_trace_read: handle was not created with BITHTM_TRACE=1"; return HTM_ERR_STATE; }
    const int64_t n = (int64_t)8 * 4096 * 2;
    if (count < n) { h->err = "htm_trace_read: buffer too small"; return HTM_ERR_ARGUMENT; }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(dst, h->d.trace, (size_t)n * 8, hipMemcpyDeviceToHost));
    return n;
}

extern "C" int htm_profile_read(htm_handle *h, int32_t max_kernels, const char **names, double *total_ms, int64_t *launches) {
    if (!h) return HTM_ERR_ARGUMENT;
    if (h) flush_tail(h);
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->prof_names.size(); ++i) {
        for (auto &pr : h->prof_events[i]) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, pr.first, pr.second);
            h->prof_ms[i] += ms;
            h->prof_n[i] += 1;
            h->prof_all.push_back(pr.first);
            h->prof_all.push_back(pr.second);
        }
        h->prof_events[i].clear();
    }
    for (hipEvent_t e : h->prof_all) hipEventDestroy(e);
    h->prof_all.clear();
    int n = (int)std::min<size_t>(h->prof_names.size(), (size_t)std::max(max_kernels, 0));
    for (int i = 0; i < n; ++i) {
        if (names) names[i] = h->prof_names[i].c_str();
        if (total_ms) total_ms[i] = h->prof_ms[i];
        if (launches) launches[i] = h->prof_n[i];
    }
    for (size_t i = 0; i < h->prof_names.size(); ++i) { h->prof_ms[i] = 0; h->prof_n[i] = 0; }
    return n;
}

// ------------------------------------------------------------------------------------------
// Model groups (htm_group.h): B members of one shape, every launch of a step covering all of them
// (grid y = member).  The group enqueues on its first member's stream.

// ... htm_group_run: the step's parity, the call's modes, the form of the group's launches (GroupForm), the span, the bank table
struct GroupGraphKey {
    int p; RunModes modes; int learning; bool fuse, large, shared; int spec, span; const void *bank_tab; int n_inputs;
    auto tie() const { return std::tie(p, modes, learning, fuse, large, shared, spec, span, bank_tab, n_inputs); }
    bool operator<(const GroupGraphKey &o) const { return tie() < o.tie(); }
};

struct htm_group {
    std::vector<htm_handle *> m;
    int n;
    int device;
    hipStream_t stream;                       // the first member's
    bool mixed;                               // some member enqueues on another stream
    std::string err;
    std::vector<void *> allocs;
    std::vector<Dev> host_tab;                // what d_tab holds: each member's Dev with every select digit launched
    Dev *d_tab;
    RecDev **d_recs;                          // each member's record descriptor (htm_handle::d_rec)
    PinDev **d_pins;                          // each member's decoding descriptor (htm_handle::d_pin)
    FeedDev **d_feeds;                        // each member's feedback descriptor (htm_handle::d_feed)
    uint32_t *stage;                          // htm_group_step: [n][W] staged host inputs
    const uint32_t **stage_tab;               // ... and the bank table that points into it
    // device tables of the members' banks / record buffers, one per distinct set (graphs hold the bank table's address)
    std::map<std::vector<const uint32_t *>, const uint32_t **> bank_tabs;
    std::map<std::vector<const void *>, GrpRecArgs *> rec_tabs;
    std::map<std::vector<int32_t *>, int32_t **> pin_tabs;      // the members' decoding outputs (htm_set_run_predicted_input)
    std::map<GroupGraphKey, hipGraphExec_t> graphs;
    // pattern capture (htm_set_group_run_active_cells): each member's capture descriptor (a constant address: graphs read the rows
    // through it), filled by the setter; capturing: rows are set
    ClsCapDev *d_caps = nullptr;
    bool capturing = false;
    // stacks of groups (htm_group_pack_columns / htm_group_pool_columns; htm_group_stack.h): the link table of the call last
    // enqueued and the host rows its copy was made from
    char *link_tab = nullptr;
    size_t link_tab_bytes = 0;
    std::vector<GrpPackRow> pack_rows;
    std::vector<char> link_rows;
    // inference views (htm_create_view): some member is a view; every member aliases one set of weights (then the steps with
    // learning = 0 scan the store once per chunk of share_m members: kgrp_scan_shared, share_chunks x share_blocks blocks)
    bool has_view, shared;
    int share_m, share_chunks, share_blocks;
    // live ticks (htm_live_tick / htm_live_reset; htm_live.h), allocated by the first such call.  One staging block -- the bank of
    // the tick's rows [n][W] (copied in, or written by the encode launch), the reset flags [n], the value rows [n][max fields] --
    // with its pinned host twin, and one result block -- the likelihoods [n] of a scored tick (htm_likelihood_tick; the copy out of any
    // other tick begins behind them), rows [n], decoded pairs [n][max fields][2], vote rows [n][I] -- with its.
    struct Live {
        char *h_stage = nullptr, *d_stage = nullptr, *h_out = nullptr, *d_out = nullptr;
        size_t off_flags = 0, off_values = 0, stage_bytes = 0, off_rows = 0, off_pairs = 0, off_votes = 0, out_bytes = 0;
        const uint32_t **bank_tab = nullptr;      // the rows of the staging bank (a constant address: the graphs' key)
        htm_step_record *d_recs = nullptr;        // the members' record slots [n] ...
        GrpRecArgs *rec_args = nullptr;           // ... as kgrp_rec_begin takes them
        int32_t **vote_tab = nullptr;             // the members' vote rows (in the result block) as kgrp_pin_begin takes them
        // a classified tick (htm_classifiers_tick): its outputs best [n][H][2], dist [n][H][buckets] lie in the result block directly
        // in FRONT of the likelihoods (cls_cap bytes, grown when a tick needs more), so that the copy out stays one; its targets [n]
        // lie in the staging block directly behind what the tick copies in anyway; the members' captured patterns [n][k * WPC] and
        // the table of their capture descriptors (a constant address: the tick's graphs read the rows through it)
        size_t off_lik = 0, cls_cap = 0;
        ClsPair *cap_rows = nullptr;
        ClsCapDev *d_caps = nullptr;
    } live;
};

#define GHIPCHK(g, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (g)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return HTM_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

template <typename T>
static int galloc(htm_group *g, T **p, size_t count) {
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) { g->err = std::string("hipMalloc: ") + hipGetErrorString(e); return HTM_ERR_HIP; }
    g->allocs.push_back(q);
    *p = (T *)q;
    return 0;
}

extern "C" const char *htm_group_last_error(const htm_group *g) { return g ? g->err.c_str() : g_create_error.c_str(); }

extern "C" void htm_group_destroy(htm_group *g) {
    if (!g) return;
    hipSetDevice(g->device);
    // (the members may be gone already: nothing here touches them or their streams; hipFree waits for the device)
    for (auto &kv : g->graphs) hipGraphExecDestroy(kv.second);
    for (void *p : g->allocs) hipFree(p);
    if (g->live.h_stage) hipHostFree(g->live.h_stage);
    if (g->live.h_out) hipHostFree(g->live.h_out);
    delete g;
}

static int group_refuse(const std::string &msg, int code) {
    g_create_error = msg;
    return code;
}

// what a member must share with the first one: the shape, and every launch size derived from it (the environment's tuning
// knobs are read per handle)
static const char *group_mismatch(const htm_handle *a, const htm_handle *b) {
    if (a->cfg.input_dim != b->cfg.input_dim) return "input_dim";
    if (a->cfg.column_dim != b->cfg.column_dim) return "column_dim";
    if (a->cfg.cell_dim != b->cfg.cell_dim) return "cell_dim";
    if (a->cfg.active_columns != b->cfg.active_columns) return "active_columns";
    if (a->cfg.segment_capacity != b->cfg.segment_capacity) return "segment_capacity";
    if (a->cfg.segment_slots != b->cfg.segment_slots) return "segment_slots";
    if (a->sz.G != b->sz.G || a->sz.sp_blocks != b->sz.sp_blocks || a->sz.sel_blocks != b->sz.sel_blocks || a->sz.c256_blocks != b->sz.c256_blocks ||
        a->sz.scan_blocks != b->sz.scan_blocks || a->sz.zero_blocks != b->sz.zero_blocks || a->sz.lean_learn_blocks != b->sz.lean_learn_blocks ||
        a->sz.lean_scan_blocks != b->sz.lean_scan_blocks || a->sz.sel_passes_full != b->sz.sel_passes_full)
        return "launch sizes (tuning knobs of the environment)";
    return nullptr;
}

extern "C" int htm_group_create(htm_handle *const *members, int32_t n, htm_group **out) {
    if (!out) return group_refuse("htm_group_create: null argument", HTM_ERR_ARGUMENT);
    *out = nullptr;
    if (!members || n <= 0) return group_refuse("htm_group_create: need members and n >= 1", HTM_ERR_ARGUMENT);
    for (int i = 0; i < n; ++i)
        if (!members[i]) return group_refuse("htm_group_create: member " + std::to_string(i) + " is null", HTM_ERR_ARGUMENT);
    const htm_handle *h0 = members[0];
    for (int i = 0; i < n; ++i) {
        const htm_handle *h = members[i];
        const std::string who = "htm_group_create: member " + std::to_string(i);
        if (!h->cfg.enable_sp || !h->cfg.enable_tm) return group_refuse(who + " needs a Spatial Pooler and a Temporal Memory", HTM_ERR_STATE);
        if (h->world > 1) return group_refuse(who + " is column-sharded", HTM_ERR_STATE);
        if (h->device != h0->device) return group_refuse(who + " is on another device", HTM_ERR_STATE);
        if (const char *what = group_mismatch(h0, h)) return group_refuse(who + ": " + what + " differs from member 0's", HTM_ERR_STATE);
        for (int j = 0; j < i; ++j)
            if (members[j] == h) return group_refuse(who + " is member " + std::to_string(j) + " again", HTM_ERR_ARGUMENT);
        if (sp_is_ahead(h)) return group_refuse(who + ": the Spatial Pooler is ahead (htm_run ended with HTM_RUN_CONTINUE)", HTM_ERR_STATE);
        if (h->phase_open || h->shard_open) return group_refuse(who + " has a step open (htm_sp_phase)", HTM_ERR_STATE);
    }
    htm_group *g = new htm_group();
    g->m.assign(members, members + n);
    g->n = n;
    g->device = h0->device;
    g->stream = h0->stream;
    for (const htm_handle *h : g->m) g->mixed |= h->stream != g->stream;
    auto fail = [&](int rc) { g_create_error = g->err; htm_group_destroy(g); return rc; };
    if (hipSetDevice(g->device) != hipSuccess) { g->err = "htm_group_create: hipSetDevice failed"; return fail(HTM_ERR_HIP); }
    g->shared = true;
    for (const htm_handle *h : g->m) {
        g->has_view |= h->is_view;
        g->shared &= h->d.presyn == h0->d.presyn && h->d.perm == h0->d.perm;
    }
    g->shared = g->shared && g->has_view && h0->knob.shared_scan;
    if (g->shared) {
        // M: the members whose column bitmaps fit 64 KiB of LDS beside each other (at most GRP_SHARED_MMAX, and the knob's cap);
        // the grid: the blocks of that LDS size resident at once, at most one per 64 rows of the pool
        const size_t per = (size_t)h0->d.colwords * 4;
        int M = (int)std::min<size_t>(GRP_SHARED_MMAX, std::max<size_t>(1, (64 * 1024) / per));
        if (h0->knob.shared_members > 0) M = std::min(M, h0->knob.shared_members);
        M = std::min(M, n);
        g->share_m = M;
        g->share_chunks = (n + M - 1) / M;
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)kgrp_scan_shared, 256, (size_t)M * per) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 1;
        }
        g->share_blocks = std::max(1, std::min(h0->sz.scan_blocks, per_cu * h0->sz.cus));
    }
    g->host_tab.resize(n);
    std::vector<RecDev *> recs(n);
    std::vector<PinDev *> pins(n);
    std::vector<FeedDev *> feeds(n);
    for (int i = 0; i < n; ++i) {
        htm_handle *h = g->m[i];
        flush_tail(h);
        if (!h->d_rec && dalloc(h, &h->d_rec, 1)) { g->err = h->err; return fail(HTM_ERR_HIP); }
        if (!h->d_pin && dalloc(h, &h->d_pin, 1)) { g->err = h->err; return fail(HTM_ERR_HIP); }
        if (!h->d_feed && dalloc(h, &h->d_feed, 1)) { g->err = h->err; return fail(HTM_ERR_HIP); }      // (zeroed: no feedback)
        if (hipStreamSynchronize(h->stream) != hipSuccess) { g->err = "htm_group_create: hipStreamSynchronize failed"; return fail(HTM_ERR_HIP); }
        g->host_tab[i] = h->d;
        g->host_tab[i].sel_passes = h->sz.sel_passes_full;
        recs[i] = h->d_rec;
        pins[i] = h->d_pin;
        feeds[i] = h->d_feed;
    }
    const int W = h0->d.W;
    int rc = 0;
    rc |= galloc(g, &g->d_tab, n);
    rc |= galloc(g, &g->d_recs, n);
    rc |= galloc(g, &g->d_pins, n);
    rc |= galloc(g, &g->d_feeds, n);
    rc |= galloc(g, &g->stage, (size_t)n * W);
    rc |= galloc(g, (uint32_t ***)&g->stage_tab, n);
    if (rc) return fail(HTM_ERR_HIP);
    std::vector<const uint32_t *> stage_rows(n);
    for (int i = 0; i < n; ++i) stage_rows[i] = g->stage + (size_t)i * W;
    // (the words of a staged row beyond ceil(input_dim / 32) stay zero)
    if (hipMemset(g->stage, 0, (size_t)n * W * 4) != hipSuccess ||
        hipMemcpy(g->d_tab, g->host_tab.data(), (size_t)n * sizeof(Dev), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_recs, recs.data(), (size_t)n * sizeof(RecDev *), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_pins, pins.data(), (size_t)n * sizeof(PinDev *), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->d_feeds, feeds.data(), (size_t)n * sizeof(FeedDev *), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy((void *)g->stage_tab, stage_rows.data(), (size_t)n * sizeof(uint32_t *), hipMemcpyHostToDevice) != hipSuccess) {
        g->err = std::string("htm_group_create: ") + hipGetErrorString(hipGetLastError());
        return fail(HTM_ERR_HIP);
    }
    *out = g;
    return HTM_OK;
}

// the device table of one set of pointers (kept: graphs hold the address of a bank table)
template <typename T, typename K>
static int group_table(htm_group *g, std::map<K, T *> &tabs, const K &key, const T *rows, T **out) {
    auto it = tabs.find(key);
    if (it == tabs.end()) {
        T *t = nullptr;
        if (galloc(g, &t, g->n)) return HTM_ERR_HIP;
        GHIPCHK(g, hipMemcpy((void *)t, rows, (size_t)g->n * sizeof(T), hipMemcpyHostToDevice));
        it = tabs.emplace(key, t).first;
    }
    *out = it->second;
    return 0;
}

// How the group's steps are launched: the form of the tail and the scan's speculation, from the most conservative member
struct GroupForm { bool fuse, large, shared; int spec; };

static GroupForm group_form(htm_group *g) {
    int lo = 1 << 30, hi = 0;
    for (int i = 0; i < g->n; ++i) {
        htm_handle *h = g->m[i];
        refresh_seg_hint(h);
        lo = std::min(lo, h->seg_hint);
        hi = std::max(hi, h->seg_hint);
    }
    const htm_handle *h0 = g->m[0];
    GroupForm f;
    f.large = h0->knob.scan_large >= 0 ? h0->knob.scan_large != 0 : hi > h0->knob.scan_large_above;
    f.fuse = h0->knob.fuse_tm && !f.large && bitmap_fits_lds(h0->d);
    f.spec = std::min(lo / SCAN_SEGS, h0->sz.scan_blocks) & ~63;
    f.shared = false;                               // (set by the caller for a step without learning)
    return f;
}

static decltype(&kgrp_learn<1>) const kt_grp_learn[4] = {kgrp_learn<1>, kgrp_learn<2>, kgrp_learn<4>, kgrp_learn<8>};
static decltype(&kgrp_tail<1>) const kt_grp_tail[4] = {kgrp_tail<1>, kgrp_tail<2>, kgrp_tail<4>, kgrp_tail<8>};
static decltype(&kgrp_scan<true, 1>) const kt_grp_scan[4] = {kgrp_scan<true, 1>, kgrp_scan<false, 1>, kgrp_scan<true, 6>, kgrp_scan<false, 6>};

// one step of every member (parity p): the one-role-per-launch schedule of enqueue_rest, unfused (htm_group.h)
static void group_enqueue_step(htm_group *g, RunModes m, const uint32_t *const *banks, int n_inputs, int learning, int p, const GroupForm &f,
                               const ClsCapDev *caps = nullptr) {
    htm_handle *h = g->m[0];                   // (launch sizes and profiling: the members' are equal)
    const Dev &d = h->d;
    const hipStream_t s = g->stream;
    const int B = g->n;
    const Dev *tab = g->d_tab;
    const dim3 g_sp(h->sz.sp_blocks, B), g_sel(h->sz.sel_blocks, B), g_256(h->sz.c256_blocks, B);
    LAUNCH_ON(h, s, 0, "group:sp_overlap", kgrp_overlap, g_sp, RB, tab, banks, n_inputs, h->sz.G, p);
    for (int pass = 1; pass < h->sz.sel_passes_full; ++pass) LAUNCH_ON(h, s, 0, "group:sp_select", kgrp_select, g_sel, RB, tab, pass, p);
    LAUNCH_ON(h, s, 0, "group:sp_count", kgrp_count, g_256, 256, tab, p);
    LAUNCH_ON(h, s, 0, "group:sp_emit", kgrp_emit, g_256, 256, tab, p);
    const int n_cls = learning ? kClassifyBlocks : 0, n_rows = learning ? d.k : 0;
    const int rows_mid = f.fuse ? 0 : n_rows, rows_tail = f.fuse ? n_rows : 0;
    const dim3 g_mid(1 + n_cls + rows_mid + h->sz.zero_blocks, B);
    LAUNCH_ON(h, s, 0, "group:tm_mid", kgrp_middle, g_mid, 256, tab, p, learning, n_cls, banks, n_inputs, rows_mid);
    const int epl = learn_epl(d);
    if (f.fuse && !f.shared) {
        const LearnScan ls = learn_scan(h);         // (but the group's speculation: its most conservative member's, group_form)
        const dim3 g_tail(ls.blocks() + rows_tail, B);
        LAUNCH_ON(h, s, ls.lds, rows_tail ? "group:tm_learn+tm_scan+sp_learn" : "group:tm_learn+tm_scan", kt_grp_tail[ls.slot], g_tail, 256, tab, p,
                  ls.n_learn, ls.n_scan, f.spec, banks, n_inputs);
    } else {
        // (f.shared: every member's learning role -- with learning = 0 the previous scan's per-cell maxima cleared, nothing else --
        // then ONE pass over the shared store for each chunk of share_m members: htm_group.h)
        LAUNCH_ON(h, s, learn_lds(epl), "group:tm_learn", kt_grp_learn[epl_slot(d)], dim3(kLearnBlocks, B), RB, tab, p);
        if (f.shared) {
            LAUNCH_ON(h, s, (size_t)g->share_m * d.colwords * 4, "group:tm_scan_shared", kgrp_scan_shared, dim3(g->share_blocks, g->share_chunks), 256, tab, B,
                      g->share_m, p);
        } else {
            const bool use_lds = bitmap_fits_lds(d);
            LAUNCH_ON(h, s, scan_lds(d, use_lds), f.large ? "group:tm_scan_large" : "group:tm_scan", kt_grp_scan[scan_slot(f.large, use_lds)], dim3(h->sz.scan_blocks, B), 256,
                      tab, p, f.spec);
        }
    }
    if (m.recording) {
        const dim3 g_rec(rec_blocks(d), B);
        LAUNCH_ON(h, s, 0, "group:record", kgrp_rec_step, g_rec, 256, tab, p, g->d_recs);
    }
    // the members' active-cell words, directly behind the record launch (htm_classifier.h); nothing outside a capturing call
    // (caps: the table of a live tick; the group's own otherwise)
    if (m.capturing) LAUNCH_ON(h, s, 0, "group:active_cells", kgcls_capture, dim3(cap_blocks(d), B), 256, tab, p, g->d_recs, caps ? caps : (const ClsCapDev *)g->d_caps);
    if (m.decoding) {
        const dim3 g_pin(pin_blocks(d.C), B);
        LAUNCH_ON(h, s, 0, "group:predicted_input", kgrp_pin_step, g_pin, 256, tab, p, g->d_pins);
    }
    if (m.feeding) {                              // (members without feedback leave both launches at once: htm_forecast.h)
        const dim3 g_pin(pin_blocks(d.C), B);
        LAUNCH_ON(h, s, 0, "group:feedback_votes", kgrp_feed_votes, g_pin, 256, tab, p, g->d_feeds);
        LAUNCH_ON(h, s, 0, "group:feedback_encode", kgrp_feed_step, dim3(1, B), ENC_THREADS, tab, p, g->d_feeds);
    }
}

// every refusal of a group call, before anything is enqueued
static int group_check(htm_group *g, const uint32_t *const *banks, const htm_run_record *records, int n_inputs = 1, int learning = 0) {
    const htm_handle *h0 = g->m[0];
    for (int i = 0; i < g->n; ++i) {
        const htm_handle *h = g->m[i];
        const std::string who = "member " + std::to_string(i);
        if (sp_is_ahead(h)) { g->err = who + ": the Spatial Pooler is ahead (htm_run ended with HTM_RUN_CONTINUE)"; return HTM_ERR_STATE; }
        if (h->shard_open) { g->err = who + " has a step open"; return HTM_ERR_STATE; }
        if (h->reset_bits) { g->err = who + " has run reset bits set (htm_set_run_resets): sequence resets inside a group run are not available"; return HTM_ERR_STATE; }
        if (h->cap_out) { g->err = who + " has active-cell rows set (htm_set_run_active_cells): pattern capture inside a group call is not available"; return HTM_ERR_STATE; }
        if ((h->step_host & 1) != (h0->step_host & 1)) {
            g->err = who + " is at step " + std::to_string(h->step_host) + ", member 0 at step " + std::to_string(h0->step_host) +
                     ": a group steps members of the same step parity only";
            return HTM_ERR_STATE;
        }
        if (banks && !banks[i]) { g->err = who + ": null bank"; return HTM_ERR_ARGUMENT; }
        if (h->feed_bank) {                         // (htm_set_run_feedback: the refusals of htm_run)
            if (!banks || h->feed_bank != banks[i] || h->feed_n != n_inputs) { g->err = who + ": run feedback was set for another bank or n_inputs (htm_set_run_feedback)"; return HTM_ERR_ARGUMENT; }
            if (learning) { g->err = who + ": run feedback is set (htm_set_run_feedback): learning must be 0"; return HTM_ERR_ARGUMENT; }
        }
        if (h->is_view) {
            std::lock_guard<std::mutex> lock(g_shared_mutex);
            if (h->shared->parent && sp_is_ahead(h->shared->parent)) { g->err = who + ": the view's parent is ahead (HTM_RUN_CONTINUE)"; return HTM_ERR_STATE; }
        }
        if (records) { int rc = check_run_record(records[i], who, g->err); if (rc) return rc; }
    }
    if (records && h0->d.C >= (1 << 24)) { g->err = "recorded group calls need column_dim below 2^24"; return HTM_ERR_STATE; }
    return 0;
}

// the members' own work first: their held-back tails and open phases, on their streams.  (A member on another stream than the
// group's: the host waits for that stream here, and for the group's stream at the end of the call.)
static int group_join(htm_group *g) {
    for (htm_handle *h : g->m) {
        flush_tail(h);
        if (int rc = view_enter(h, 0)) { g->err = h->err; return rc; }
        if (close_open_phases(h)) { g->err = h->err; return HTM_ERR_HIP; }
        if (h->stream != g->stream) GHIPCHK(g, hipStreamSynchronize(h->stream));
    }
    // a member whose epsilon changed since the table was written (htm_set_epsilon): the table again
    bool stale = false;
    for (int i = 0; i < g->n; ++i) stale |= g->host_tab[i].eps != g->m[i]->d.eps;
    if (stale) {
        for (int i = 0; i < g->n; ++i) g->host_tab[i].eps = g->m[i]->d.eps;
        GHIPCHK(g, hipStreamSynchronize(g->stream));
        GHIPCHK(g, hipMemcpy(g->d_tab, g->host_tab.data(), (size_t)g->n * sizeof(Dev), hipMemcpyHostToDevice));
    }
    return 0;
}

// The setup of a group call's modes, on the members' tables: the record and decoding descriptors of every member filled by one
// begin launch each (begin_run_modes is a single handle's)
static int group_begin_modes(htm_group *g, int n_steps, const htm_run_record *records, RunModes *modes) {
    const int B = g->n;
    htm_handle *h0 = g->m[0];
    const hipStream_t s = g->stream;
    if (records) {
        std::vector<GrpRecArgs> rows(B);
        std::vector<const void *> key;
        for (int i = 0; i < B; ++i) {
            rows[i] = GrpRecArgs{records[i].records, records[i].active_column, records[i].column_prediction};
            key.insert(key.end(), {rows[i].rec, rows[i].cols, rows[i].colpred});
        }
        GrpRecArgs *args = nullptr;
        if (int rc = group_table(g, g->rec_tabs, key, rows.data(), &args)) return rc;
        LAUNCH_ON(h0, s, 0, "group:record", kgrp_rec_clear, B, 64, g->d_recs);
        LAUNCH_ON(h0, s, 0, "group:record", kgrp_rec_begin, dim3(rec_blocks(h0->d), B), 256, g->d_tab, (int)((h0->step_host + 1) & 1), g->d_recs, args, n_steps);
    }
    // members with decoding outputs (htm_set_run_predicted_input): their rows zeroed and every member's descriptor filled (the
    // others' with no rows), then one decoding launch behind each step
    std::vector<int32_t *> outs(B);
    for (int i = 0; i < B; ++i) outs[i] = g->m[i]->pin_out;
    const bool decoding = std::any_of(outs.begin(), outs.end(), [](int32_t *o) { return o != nullptr; });
    if (decoding) {
        int32_t **out_tab = nullptr;
        if (int rc = group_table(g, g->pin_tabs, outs, outs.data(), &out_tab)) return rc;
        LAUNCH_ON(h0, s, 0, "group:predicted_input", kgrp_pin_begin, dim3(pin_begin_blocks(n_steps, h0->d.I), B), 256, g->d_tab, (int)((h0->step_host + 1) & 1), g->d_pins, out_tab, n_steps);
    }
    const bool feeding = std::any_of(g->m.begin(), g->m.end(), [](const htm_handle *h) { return h->feed_bank != nullptr; });
    *modes = RunModes{records != nullptr, false, decoding, feeding, records != nullptr && g->capturing};
    return 0;
}

static int group_run(htm_group *g, const uint32_t **bank_tab, int n_inputs, int n_steps, int learning, int use_graph,
                     const htm_run_record *records) {
    htm_handle *h0 = g->m[0];
    const hipStream_t s = g->stream;
    learning = learning ? 1 : 0;
    RunModes modes;
    if (int rc = group_begin_modes(g, n_steps, records, &modes)) return rc;
    GroupForm f = group_form(g);
    f.shared = g->shared && !learning;
    const bool graph = run_schedule(h0, n_steps, use_graph).graph;
    const int span_max = h0->knob.graph_steps;
    int p = (int)(h0->step_host & 1);
    for (int t = 0; t < n_steps;) {
        if (!graph) {
            group_enqueue_step(g, modes, bank_tab, n_inputs, learning, p, f);
            p ^= 1;
            t += 1;
            continue;
        }
        const int span = n_steps - t >= span_max ? span_max : 1;
        const GroupGraphKey key{p, modes, learning, f.fuse, f.large, f.shared, f.spec, span, bank_tab, n_inputs};
        const hipGraphExec_t exec = cached_graph(g->graphs, key, s, g->err, [&] {
            for (int i = 0; i < span; ++i) group_enqueue_step(g, modes, bank_tab, n_inputs, learning, (p + i) & 1, f);
            return 0;
        });
        if (!exec) return HTM_ERR_HIP;
        GHIPCHK(g, hipGraphLaunch(exec, s));
        p ^= span & 1;
        t += span;
    }
    for (htm_handle *h : g->m) {
        h->step_host += n_steps;
        h->window_known = true;                   // (every select leaves the next step's window behind)
        if (learning) weights_touched(h);
    }
    const int rc = launch_status(g->err);
    if (rc) return rc;
    // leave each member's segment count where its next call -- group or solo -- finds it, as htm_run does (no wait)
    for (htm_handle *h : g->m) GHIPCHK(g, hand_back_segments(h, &h->d.ctr->S, s));
    if (g->mixed) GHIPCHK(g, hipStreamSynchronize(s));
    return HTM_OK;
}

extern "C" int htm_group_run(htm_group *g, const uint32_t *const *device_banks, int32_t n_inputs, int32_t n_steps, int32_t learning,
                             int32_t use_graph, const htm_run_record *records) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!device_banks || n_inputs < 1 || n_steps < 0) { g->err = "htm_group_run: need device_banks, n_inputs >= 1 and n_steps >= 0"; return HTM_ERR_ARGUMENT; }
    if (learning && g->has_view) { g->err = "htm_group_run: a group with inference views steps with learning = 0 only"; return HTM_ERR_STATE; }
    int rc = group_check(g, device_banks, records, n_inputs, learning);
    if (rc) return rc;
    if (g->capturing && !records) { g->err = "htm_group_run: active-cell rows are set (htm_set_group_run_active_cells): only a recorded run fills them"; return HTM_ERR_ARGUMENT; }
    if (n_steps == 0) return rc;
    GHIPCHK(g, hipSetDevice(g->device));
    rc = group_join(g);
    if (rc) return rc;
    std::vector<const uint32_t *> key(device_banks, device_banks + g->n);
    const uint32_t **tab = nullptr;
    rc = group_table(g, g->bank_tabs, key, key.data(), &tab);
    if (rc) return rc;
    return group_run(g, tab, n_inputs, n_steps, learning, use_graph, records);
}

extern "C" int htm_group_step(htm_group *g, const uint32_t *packed_inputs, int32_t learning, const htm_run_record *records) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!packed_inputs) { g->err = "htm_group_step: null packed_inputs"; return HTM_ERR_ARGUMENT; }
    if (learning && g->has_view) { g->err = "htm_group_step: a group with inference views steps with learning = 0 only"; return HTM_ERR_STATE; }
    int rc = group_check(g, nullptr, records);
    if (rc) return rc;
    if (g->capturing && !records) { g->err = "htm_group_step: active-cell rows are set (htm_set_group_run_active_cells): only a recorded step fills them"; return HTM_ERR_ARGUMENT; }
    GHIPCHK(g, hipSetDevice(g->device));
    rc = group_join(g);
    if (rc) return rc;
    // the rows into the staging bank, W words apart (as stage_input: the copy has read the caller's words when it returns)
    const Dev &d = g->m[0]->d;
    const size_t words = (size_t)(d.I + 31) / 32;
    GHIPCHK(g, hipMemcpy2DAsync(g->stage, (size_t)d.W * 4, packed_inputs, words * 4, words * 4, g->n, hipMemcpyHostToDevice, g->stream));
    return group_run(g, g->stage_tab, 1, 1, learning, 0, records);
}

// Pattern capture of the group's recorded calls (htm_classifier.h, kgcls_capture): the members' rows go into the group's table of
// capture descriptors with one copy on the group's stream, from the call's own words (read when the copy returns) -- the runs that
// follow, and the graphs they replay, read the rows through the table.  NULL clears them.
extern "C" int htm_set_group_run_active_cells(htm_group *g, void *const *device_pairs) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!device_pairs) { g->capturing = false; return HTM_OK; }
    for (int i = 0; i < g->n; ++i) {
        if (!device_pairs[i]) { g->err = "htm_set_group_run_active_cells: member " + std::to_string(i) + ": null rows"; return HTM_ERR_ARGUMENT; }
        if (int rc = pin_refuse(g->m[i], "htm_set_group_run_active_cells")) { g->err = "member " + std::to_string(i) + ": " + g->m[i]->err; return rc; }
    }
    GHIPCHK(g, hipSetDevice(g->device));
    if (!g->d_caps && galloc(g, &g->d_caps, (size_t)g->n)) return HTM_ERR_HIP;
    std::vector<ClsCapDev> caps((size_t)g->n);
    for (int i = 0; i < g->n; ++i) caps[i].rows = (ClsPair *)device_pairs[i];
    GHIPCHK(g, hipMemcpyAsync(g->d_caps, caps.data(), caps.size() * sizeof(ClsCapDev), hipMemcpyHostToDevice, g->stream));
    g->capturing = true;
    return HTM_OK;
}

// ------------------------------------------------------------------------------------------
// Stacks of model groups (htm_group_stack.h): the links of B streams' hierarchies, every launch covering all
// members (grid y = member).  A call's per-member pointers go into the group's link table -- one buffer, grown when a call needs
// more, filled by ONE copy on the group's stream from a vector the group keeps (the copy has read it when it returns; the launches
// behind it on the stream read the table, and the next call's copy orders itself behind them).

// what both entries refuse about the group's members, before anything is enqueued
static int gstack_check(htm_group *g, const char *what) {
    if (g->n > GSTACK_MAX_MEMBERS) { g->err = std::string(what) + ": more than 65535 members"; return HTM_ERR_ARGUMENT; }
    for (int i = 0; i < g->n; ++i) {
        const htm_handle *h = g->m[i];
        const std::string who = std::string(what) + ": member " + std::to_string(i);
        if (!h->cfg.enable_sp) { g->err = who + " needs the device's own Spatial Pooler (its input rows are packed)"; return HTM_ERR_STATE; }
        if (h->world > 1) { g->err = who + " is column-sharded"; return HTM_ERR_STATE; }
        if (sp_is_ahead(h)) { g->err = who + ": the Spatial Pooler is ahead (htm_run ended with HTM_RUN_CONTINUE)"; return HTM_ERR_STATE; }
        if (h->stream != g->stream) { g->err = who + " enqueues on another stream than the group's"; return HTM_ERR_STATE; }
    }
    return 0;
}

// the group's link table with room for `bytes`, filled from `rows` by one copy on the group's stream
static int gstack_table(htm_group *g, const void *rows, size_t bytes, char **out) {
    if (g->link_tab_bytes < bytes) {
        char *t = nullptr;
        if (galloc(g, &t, bytes)) return HTM_ERR_HIP;       // (the old one stays in g->allocs until the group goes: launches may still read it)
        g->link_tab = t;
        g->link_tab_bytes = bytes;
    }
    GHIPCHK(g, hipMemcpyAsync(g->link_tab, rows, bytes, hipMemcpyHostToDevice, g->stream));
    *out = g->link_tab;
    return 0;
}

extern "C" int htm_group_pack_columns(htm_group *g, const int32_t *const *device_lists, int32_t k, int32_t n_rows, int32_t stride,
                                      uint32_t *const *device_banks, int32_t bank_rows, const int32_t *first_rows) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!device_lists || !device_banks || !first_rows) { g->err = "htm_group_pack_columns: null lists, banks or first_rows"; return HTM_ERR_ARGUMENT; }
    if (k < 1 || stride < 1 || n_rows < 0 || bank_rows < 1) {
        g->err = "htm_group_pack_columns: k >= 1, stride >= 1, n_rows >= 0 and bank_rows >= 1";
        return HTM_ERR_ARGUMENT;
    }
    if (g->n > GSTACK_MAX_MEMBERS) { g->err = "htm_group_pack_columns: more than 65535 members"; return HTM_ERR_ARGUMENT; }
    for (int i = 0; i < g->n; ++i) {
        const std::string who = "htm_group_pack_columns: member " + std::to_string(i);
        if (!device_lists[i] || !device_banks[i]) { g->err = who + ": null lists or bank"; return HTM_ERR_ARGUMENT; }
        if (first_rows[i] < 0 || first_rows[i] >= bank_rows) { g->err = who + ": 0 <= first_row < bank_rows"; return HTM_ERR_ARGUMENT; }
        if (((uintptr_t)device_banks[i] & 15) != 0) { g->err = who + ": the bank must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    }
    if (int rc = gstack_check(g, "htm_group_pack_columns")) return rc;
    htm_handle *h0 = g->m[0];
    if (pack_lds(h0->d) > PACK_LDS_MAX) { g->err = "htm_group_pack_columns: an input row of the members does not fit the LDS (input_dim above 524288)"; return HTM_ERR_ARGUMENT; }
    if (n_rows == 0) return HTM_OK;
    GHIPCHK(g, hipSetDevice(g->device));
    g->pack_rows.resize((size_t)g->n);
    for (int i = 0; i < g->n; ++i) g->pack_rows[i] = GrpPackRow{device_lists[i], device_banks[i], first_rows[i], 0};
    char *tab = nullptr;
    if (int rc = gstack_table(g, g->pack_rows.data(), (size_t)g->n * sizeof(GrpPackRow), &tab)) return rc;
    LAUNCH_ON(h0, g->stream, pack_lds(h0->d), "group:pack_columns", kgrp_pack_columns, dim3(n_rows, g->n), PACK_THREADS, (const Dev *)g->d_tab,
              (const GrpPackRow *)tab, 0ll, k, stride, bank_rows);
    return launch_status(g->err);
}

// The scratch: member m's part begins m * per_batch * (stride + 8) * 4 W bytes in, per_batch = floor(scratch_bytes / (B * (stride
// + 8) * 4 W)) windows; inside it, the batch's per_batch * stride bitmap rows, then its per_batch snapshot rows (htm_pool.h).  The
// table: B PoolDev of the whole call, then B GrpPackRow of the pack launches into the bitmap rows -- one copy.
extern "C" int htm_group_pool_columns(htm_group *g, htm_pool_link link, const int32_t *const *device_lists, int32_t k,
                                      const uint32_t *const *device_column_prediction, int32_t n_rows, uint8_t *const *device_persistence,
                                      uint32_t *const *device_prev, const uint32_t *const *device_reset_bits, void *device_scratch, int64_t scratch_bytes,
                                      uint32_t *const *device_banks, int32_t bank_rows, const int32_t *first_rows) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!device_lists || !device_banks || !first_rows || !device_column_prediction || !device_persistence || !device_prev || !device_scratch) {
        g->err = "htm_group_pool_columns: null lists, banks, first_rows, column predictions, state or scratch";
        return HTM_ERR_ARGUMENT;
    }
    if (link.struct_bytes != sizeof(htm_pool_link)) { g->err = "htm_group_pool_columns: struct_bytes != sizeof(htm_pool_link)"; return HTM_ERR_ARGUMENT; }
    if (k < 1 || link.stride < 1 || n_rows < 0 || bank_rows < 1) {
        g->err = "htm_group_pool_columns: k >= 1, stride >= 1, n_rows >= 0 and bank_rows >= 1";
        return HTM_ERR_ARGUMENT;
    }
    if (link.active_weight < 0 || link.active_weight > 255 || link.predicted_weight < 0 || link.predicted_weight > 255 ||
        (link.active_weight == 0 && link.predicted_weight == 0)) {
        g->err = "htm_group_pool_columns: 0 <= active_weight, predicted_weight <= 255, not both 0";
        return HTM_ERR_ARGUMENT;
    }
    if (link.decay < 1 || link.decay > 255 || link.ceiling < 1 || link.ceiling > 255) {
        g->err = "htm_group_pool_columns: 1 <= decay <= 255 and 1 <= ceiling <= 255";
        return HTM_ERR_ARGUMENT;
    }
    if (g->n > GSTACK_MAX_MEMBERS) { g->err = "htm_group_pool_columns: more than 65535 members"; return HTM_ERR_ARGUMENT; }
    if (((uintptr_t)device_scratch & 15) != 0) { g->err = "htm_group_pool_columns: the scratch must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
    for (int i = 0; i < g->n; ++i) {
        const std::string who = "htm_group_pool_columns: member " + std::to_string(i);
        if (!device_lists[i] || !device_banks[i] || !device_column_prediction[i] || !device_persistence[i] || !device_prev[i]) {
            g->err = who + ": null lists, bank, column prediction or state";
            return HTM_ERR_ARGUMENT;
        }
        if (first_rows[i] < 0 || first_rows[i] >= bank_rows) { g->err = who + ": 0 <= first_row < bank_rows"; return HTM_ERR_ARGUMENT; }
        if (((uintptr_t)device_banks[i] & 15) != 0) { g->err = who + ": the bank must be 16-byte aligned"; return HTM_ERR_ARGUMENT; }
        if ((((uintptr_t)device_persistence[i] | (uintptr_t)device_prev[i]) & 15) != 0) {
            g->err = who + ": the persistence and the prev words must be 16-byte aligned";
            return HTM_ERR_ARGUMENT;
        }
    }
    if (int rc = gstack_check(g, "htm_group_pool_columns")) return rc;
    htm_handle *h0 = g->m[0];
    const int C = h0->d.I, W = h0->d.W, B = g->n;
    if (C > POOL_MAX_COLUMNS) { g->err = "htm_group_pool_columns: more lower columns (the members' input_dim) than HTM_POOL_MAX_COLUMNS (262144)"; return HTM_ERR_ARGUMENT; }
    if (link.union_bits < 1 || link.union_bits > C) { g->err = "htm_group_pool_columns: 1 <= union_bits <= the members' input_dim"; return HTM_ERR_ARGUMENT; }
    const size_t window = pool_window_bytes(W, link.stride);
    if (scratch_bytes < 0 || (uint64_t)scratch_bytes / window < (uint64_t)B) {
        g->err = "htm_group_pool_columns: the scratch is too small for one window of every member (" + std::to_string(window) + " bytes each)";
        return HTM_ERR_ARGUMENT;
    }
    if (n_rows == 0) return HTM_OK;
    GHIPCHK(g, hipSetDevice(g->device));
    // (a batch's steps are the pack launch's grid: 32-bit)
    const int per_batch = (int)std::min<uint64_t>(std::min<uint64_t>((uint64_t)n_rows, (uint64_t)scratch_bytes / ((uint64_t)B * window)), (uint64_t)(INT32_MAX / link.stride));
    const int PW = (C + 31) / 32;
    const size_t member_bytes = gpool_member_bytes(W, link.stride, per_batch);
    const size_t pool_bytes = (size_t)B * sizeof(PoolDev), bytes = pool_bytes + (size_t)B * sizeof(GrpPackRow);
    g->link_rows.resize(bytes);
    PoolDev *pools = (PoolDev *)g->link_rows.data();
    GrpPackRow *packs = (GrpPackRow *)(g->link_rows.data() + pool_bytes);
    for (int i = 0; i < B; ++i) {
        char *part = (char *)device_scratch + (size_t)i * member_bytes;
        PoolDev a;
        a.C = C; a.W = W; a.PW = PW;
        a.stride = link.stride; a.n_windows = n_rows;
        a.active_weight = link.active_weight; a.predicted_weight = link.predicted_weight; a.decay = link.decay; a.ceiling = link.ceiling;
        a.union_bits = link.union_bits;
        a.bank_rows = bank_rows; a.first_row = first_rows[i];
        a.bitmaps = (const uint32_t *)part;
        a.colpred = device_column_prediction[i];
        a.resets = device_reset_bits ? device_reset_bits[i] : nullptr;
        a.persistence = device_persistence[i]; a.prev = device_prev[i];
        a.snap = (uint8_t *)part + (size_t)per_batch * (size_t)link.stride * (size_t)W * 4;      // (a multiple of 16 bytes: W is a multiple of 4)
        a.bank = device_banks[i];
        pools[i] = a;
        packs[i] = GrpPackRow{device_lists[i], (uint32_t *)part, 0, 0};
    }
    char *tab = nullptr;
    if (int rc = gstack_table(g, g->link_rows.data(), bytes, &tab)) return rc;
    const PoolDev *d_pools = (const PoolDev *)tab;
    const GrpPackRow *d_packs = (const GrpPackRow *)(tab + pool_bytes);
    for (long long r0 = 0; r0 < n_rows; r0 += per_batch) {
        const int n = (int)std::min<long long>(per_batch, n_rows - r0);
        const long long steps = (long long)n * link.stride, first_step = r0 * link.stride;
        // the bitmap rows: one per step, row s of the member's part (bank_rows = the batch's steps, no rotation)
        LAUNCH_ON(h0, g->stream, pack_lds(h0->d), "group:pool_pack", kgrp_pack_columns, dim3((int)steps, B), PACK_THREADS, (const Dev *)g->d_tab, d_packs,
                  first_step * (long long)k, k, 1, (int)steps);
        LAUNCH_ON(h0, g->stream, 0, "group:pool_scan", kgpool_scan, dim3((W * 32 + POOL_THREADS - 1) / POOL_THREADS, B), POOL_THREADS, d_pools, (int)r0, n);
        LAUNCH_ON(h0, g->stream, pool_select_lds(W), "group:pool_select", kgpool_select, dim3(n, B), POOL_THREADS, d_pools, (int)r0, n);
    }
    return launch_status(g->err);
}

// ------------------------------------------------------------------------------------------
// Anomaly likelihood (htm_likelihood.h): the state of n streams in ONE device allocation, laid out as
// htm_likelihood_export hands it out -- t int64[n], mean double[n], std double[n], flag int32[n] (padded to 8 bytes),
// q ring int32[n][window], a ring int32[n][history] (padded to 8 bytes) -- the tail table, and the device's pointer table of a
// call over more than one stream.  The object keeps nothing of the handles its calls come through: no stream, no event.
struct htm_likelihood {
    int device = 0, n = 0;
    LikDev d;
    char *state = nullptr;
    size_t bytes = 0;
    double *tail = nullptr;
    const htm_step_record **d_tab = nullptr;  // [n] device pointers: the records of the update last enqueued
    int32_t *d_flags = nullptr;               // htm_likelihood_reset's flags [n]
};

static int lik_refuse(htm_handle *h, const std::string &msg, int code) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

extern "C" void htm_likelihood_destroy(htm_likelihood *lk) {
    if (!lk) return;
    hipSetDevice(lk->device);
    if (lk->state) hipFree(lk->state);        // (hipFree waits for the device: nothing enqueued still reads them)
    if (lk->tail) hipFree(lk->tail);
    if (lk->d_tab) hipFree((void *)lk->d_tab);
    if (lk->d_flags) hipFree(lk->d_flags);
    delete lk;
}

extern "C" int htm_likelihood_create(htm_handle *h, const htm_likelihood_config *cfg, const double *tail_table513, int32_t n_streams, htm_likelihood **out) {
    if (out) *out = nullptr;
    if (!h || !cfg || !tail_table513 || !out) return lik_refuse(h, "htm_likelihood_create: null argument", HTM_ERR_ARGUMENT);
    if (cfg->struct_bytes != sizeof(htm_likelihood_config)) return lik_refuse(h, "htm_likelihood_create: htm_likelihood_config size mismatch", HTM_ERR_ARGUMENT);
    if (cfg->learning_period < 0 || cfg->estimation_samples < 1 || cfg->history < 1 || cfg->history > HTM_LIKELIHOOD_MAX_HISTORY ||
        cfg->averaging_window < 1 || cfg->averaging_window > HTM_LIKELIHOOD_MAX_WINDOW || cfg->reestimation_period < 1)
        return lik_refuse(h, "htm_likelihood_create: learning_period >= 0, estimation_samples >= 1, history in [1, 16384], averaging_window in [1, 64], "
                             "reestimation_period >= 1", HTM_ERR_ARGUMENT);
    if (n_streams < 1) return lik_refuse(h, "htm_likelihood_create: n_streams must be at least 1", HTM_ERR_ARGUMENT);
    if (h->world > 1) return lik_refuse(h, "htm_likelihood_create: not available on a column-sharded handle", HTM_ERR_STATE);
    HIPCHK(h, hipSetDevice(h->device));
    htm_likelihood *lk = new htm_likelihood();
    lk->device = h->device;
    lk->n = n_streams;
    const size_t n = (size_t)n_streams;
    const size_t off_mean = n * 8, off_std = n * 16, off_flag = n * 24, off_q = (off_flag + n * 4 + 7) & ~(size_t)7;
    const size_t off_a = off_q + n * (size_t)cfg->averaging_window * 4;
    lk->bytes = (off_a + n * (size_t)cfg->history * 4 + 7) & ~(size_t)7;
    bool ok = hipMalloc((void **)&lk->state, lk->bytes) == hipSuccess && hipMalloc((void **)&lk->tail, HTM_LIKELIHOOD_TAIL * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&lk->d_tab, n * sizeof(void *)) == hipSuccess && hipMalloc((void **)&lk->d_flags, n * sizeof(int32_t)) == hipSuccess;
    // (synchronous: the state and the table are there when the call returns, whatever stream the first update comes on)
    ok = ok && hipMemset(lk->state, 0, lk->bytes) == hipSuccess &&
         hipMemcpy(lk->tail, tail_table513, HTM_LIKELIHOOD_TAIL * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        htm_likelihood_destroy(lk);
        return lik_refuse(h, "htm_likelihood_create: device allocation failed", HTM_ERR_HIP);
    }
    lk->d.p = LikParams{cfg->learning_period, cfg->estimation_samples, cfg->history, cfg->averaging_window, cfg->reestimation_period};
    lk->d.t = (int64_t *)lk->state;
    lk->d.mean = (double *)(lk->state + off_mean);
    lk->d.std = (double *)(lk->state + off_std);
    lk->d.flag = (int32_t *)(lk->state + off_flag);
    lk->d.q_ring = (int32_t *)(lk->state + off_q);
    lk->d.a_ring = (int32_t *)(lk->state + off_a);
    lk->d.tail = lk->tail;
    *out = lk;
    return HTM_OK;
}

// what every call on an existing object checks of its handle
static int lik_check(const char *what, htm_likelihood *lk, htm_handle *h) {
    if (!lk || !h) return lik_refuse(h, std::string(what) + ": null argument", HTM_ERR_ARGUMENT);
    if (h->world > 1) return lik_refuse(h, std::string(what) + ": not available on a column-sharded handle", HTM_ERR_STATE);
    if (h->device != lk->device) return lik_refuse(h, std::string(what) + ": the handle is on another device than the likelihood object", HTM_ERR_ARGUMENT);
    return 0;
}

extern "C" int64_t htm_likelihood_state_bytes(const htm_likelihood *lk) { return lk ? (int64_t)lk->bytes : (int64_t)HTM_ERR_ARGUMENT; }

extern "C" int htm_likelihood_update(htm_likelihood *lk, htm_handle *h, const htm_step_record *const *device_records, int32_t n_steps, double *device_out) {
    if (int rc = lik_check("htm_likelihood_update", lk, h)) return rc;
    if (!device_records || !device_out) return lik_refuse(h, "htm_likelihood_update: null records or output", HTM_ERR_ARGUMENT);
    if (n_steps < 0) return lik_refuse(h, "htm_likelihood_update: n_steps must not be negative", HTM_ERR_ARGUMENT);
    for (int i = 0; i < lk->n; ++i)
        if (!device_records[i]) return lik_refuse(h, "htm_likelihood_update: stream " + std::to_string(i) + " has no records", HTM_ERR_ARGUMENT);
    if (n_steps == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(lk->device));
    const htm_step_record *const *tab = nullptr;
    if (lk->n > 1) {
        // the one copy of the pointer table, from the call's own (pageable) words: the copy has read them when it returns, as the
        // staging copy of htm_group_step, so there is no staging of the object's to protect, nothing to wait for and no stream kept
        HIPCHK(h, hipMemcpyAsync((void *)lk->d_tab, (const void *)device_records, (size_t)lk->n * sizeof(void *), hipMemcpyHostToDevice, h->stream));
        tab = lk->d_tab;
    }
    // launches of at most HTM_LIKELIHOOD_CHUNK steps each, every one over all streams
    for (int first = 0; first < n_steps; first += HTM_LIKELIHOOD_CHUNK)
        LAUNCH(h, "likelihood", klik_update, dim3(1, lk->n), HTM_LIKELIHOOD_THREADS, lk->d, tab, tab ? nullptr : device_records[0], first,
               std::min<int>(HTM_LIKELIHOOD_CHUNK, n_steps - first), (int)n_steps, device_out);
    return launch_status(h->err);
}

extern "C" int htm_likelihood_reset(htm_likelihood *lk, htm_handle *h, const uint8_t *streams) {
    if (int rc = lik_check("htm_likelihood_reset", lk, h)) return rc;
    HIPCHK(h, hipSetDevice(lk->device));
    if (streams) {                                  // (the call's own pageable words: the copy has read them when it returns)
        std::vector<int32_t> flags((size_t)lk->n);
        for (int i = 0; i < lk->n; ++i) flags[i] = streams[i] ? 1 : 0;
        HIPCHK(h, hipMemcpyAsync(lk->d_flags, flags.data(), flags.size() * 4, hipMemcpyHostToDevice, h->stream));
    }
    LAUNCH(h, "likelihood:reset", klik_reset, dim3(1, lk->n), HTM_LIKELIHOOD_THREADS, lk->d, streams ? (const int32_t *)lk->d_flags : (const int32_t *)nullptr);
    return launch_status(h->err);
}

extern "C" int htm_likelihood_export(htm_likelihood *lk, htm_handle *h, void *host_state, int64_t bytes) {
    if (int rc = lik_check("htm_likelihood_export", lk, h)) return rc;
    if (!host_state || bytes != (int64_t)lk->bytes) return lik_refuse(h, "htm_likelihood_export: need host_state of htm_likelihood_state_bytes bytes", HTM_ERR_ARGUMENT);
    HIPCHK(h, hipSetDevice(lk->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(host_state, lk->state, lk->bytes, hipMemcpyDeviceToHost));
    return HTM_OK;
}

extern "C" int htm_likelihood_import(htm_likelihood *lk, htm_handle *h, const void *host_state, int64_t bytes) {
    if (int rc = lik_check("htm_likelihood_import", lk, h)) return rc;
    if (!host_state || bytes != (int64_t)lk->bytes) return lik_refuse(h, "htm_likelihood_import: need host_state of htm_likelihood_state_bytes bytes", HTM_ERR_ARGUMENT);
    // (the values a kernel indexes with are reduced there, but a t below 0 has no meaning)
    for (int i = 0; i < lk->n; ++i)
        if (((const int64_t *)host_state)[i] < 0) return lik_refuse(h, "htm_likelihood_import: stream " + std::to_string(i) + " has t < 0", HTM_ERR_ARGUMENT);
    HIPCHK(h, hipSetDevice(lk->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(lk->state, host_state, lk->bytes, hipMemcpyHostToDevice));
    return HTM_OK;
}

// ------------------------------------------------------------------------------------------
// SDR classifier (htm_classifier.h): the weights, the ring of recent patterns, the count of patterns since the
// history was emptied and the per-step accumulators in device memory; the total step count, which names the ring's slots, on the
// host.  As the likelihood object it keeps nothing of the handles its calls come through.
struct htm_classifier {
    int device = 0;
    ClsDev d{};                                 // (of a bank: member 0's)
    ClsFrozen frozen{};                         // the frozen calls' accumulators: made by the first one, made anew when a call needs more rows
    size_t frozen_rows = 0;                     // (streams x steps of a launch x horizons) rows they hold
    int64_t total = 0;
    size_t ring_bytes = 0;                      // of one stream
    std::vector<void *> allocs;
    // a bank (htm_classifiers_create): n streams, member-major; a single object has n = 1
    int n = 1;
    bool shares = false;                        // the weights are another object's: read here, never written
    std::shared_ptr<void> weights;              // the weight block, freed with the last object that holds it
    void **d_tab = nullptr;                     // [3][n] device pointers of a call: pairs, targets, reset bits
    int32_t *d_flags = nullptr;                 // [n] the streams a reset names
};

static int cls_refuse(htm_handle *h, const std::string &msg, int code) {
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

extern "C" void htm_classifier_destroy(htm_classifier *clf) {
    if (!clf) return;
    hipSetDevice(clf->device);
    for (void *p : clf->allocs) hipFree(p);     // (hipFree waits for the device: nothing enqueued still reads them)
    delete clf;
}

// zeroed device memory of the object's, ordered on h's stream (null: the allocation failed)
template <typename T>
static T *cls_alloc(htm_classifier *clf, htm_handle *h, size_t count) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) return nullptr;
    clf->allocs.push_back(p);
    if (hipMemsetAsync(p, 0, std::max<size_t>(count, 1) * sizeof(T), h->stream) != hipSuccess) return nullptr;
    return (T *)p;
}

// the one constructor: n streams of one config, over weights of their own or (share) over the table of an existing object
static int cls_create(const std::string &what, htm_handle *h, const htm_classifier_config *cfg, const int32_t *exp_table2049, int32_t n, htm_classifier *share,
                      htm_classifier **out) {
    if (out) *out = nullptr;
    if (!h || !cfg || !exp_table2049 || !out) return cls_refuse(h, what + ": null argument", HTM_ERR_ARGUMENT);
    if (cfg->struct_bytes != sizeof(htm_classifier_config)) return cls_refuse(h, what + ": htm_classifier_config size mismatch", HTM_ERR_ARGUMENT);
    bool ok = cfg->buckets >= 1 && cfg->buckets <= HTM_CLASSIFIER_MAX_BUCKETS && cfg->n_steps >= 1 && cfg->n_steps <= HTM_CLASSIFIER_MAX_HORIZONS &&
              cfg->alpha_q >= 1 && cfg->alpha_q <= 65536 && cfg->cell_dim >= 1 && cfg->cell_dim <= 64 && cfg->units >= cfg->cell_dim &&
              cfg->units % cfg->cell_dim == 0 && cfg->max_pairs >= 1;
    for (int i = 0; ok && i < cfg->n_steps; ++i)
        ok = cfg->steps[i] >= 0 && cfg->steps[i] <= HTM_CLASSIFIER_MAX_HORIZON && (i == 0 || cfg->steps[i] > cfg->steps[i - 1]);
    if (!ok)
        return cls_refuse(h, what + ": buckets in [1, 1024], 1 to 8 ascending steps in [0, 64], alpha_q in [1, 65536], cell_dim in [1, 64], "
                             "units a positive multiple of cell_dim, max_pairs >= 1", HTM_ERR_ARGUMENT);
    if (n < 1 || n > 65535 / cfg->n_steps)
        return cls_refuse(h, what + ": n_streams must be in [1, 65535 / n_steps = " + std::to_string(65535 / cfg->n_steps) + "] (the member shares grid y with the horizon)",
                          HTM_ERR_ARGUMENT);
    if (h->world > 1) return cls_refuse(h, what + ": not available on a column-sharded handle", HTM_ERR_STATE);
    if (share) {
        const ClsDev &o = share->d;
        bool same = share->n == 1 && o.B == cfg->buckets && o.H == cfg->n_steps && o.K == cfg->cell_dim && (int64_t)o.n_cols * o.K == cfg->units &&
                    o.alpha_q == cfg->alpha_q && o.max_pairs == cfg->max_pairs;
        for (int i = 0; same && i < o.H; ++i) same = o.steps[i] == cfg->steps[i];
        if (!same) return cls_refuse(h, what + ": share_weights_of must be a one-stream classifier of the same config", HTM_ERR_ARGUMENT);
        if (share->device != h->device) return cls_refuse(h, what + ": share_weights_of lives on another device than the handle", HTM_ERR_ARGUMENT);
    }
    HIPCHK(h, hipSetDevice(h->device));
    htm_classifier *clf = new htm_classifier();
    clf->device = h->device;
    clf->n = n;
    clf->shares = share != nullptr;
    ClsDev &d = clf->d;
    d.B = cfg->buckets;
    d.B_pad = (cfg->buckets + 3) & ~3;
    d.H = cfg->n_steps;
    d.K = cfg->cell_dim;
    d.WPC = (cfg->cell_dim + 31) / 32;
    d.n_cols = cfg->units / cfg->cell_dim;
    d.alpha_q = cfg->alpha_q;
    d.max_pairs = cfg->max_pairs;
    d.ring_len = cfg->steps[cfg->n_steps - 1] + 1;
    for (int i = 0; i < d.H; ++i) d.steps[i] = cfg->steps[i];
    d.w_stride = (int64_t)cfg->units * d.B_pad;
    clf->ring_bytes = (size_t)d.ring_len * d.max_pairs * sizeof(ClsPair);
    const size_t N = (size_t)n;
    if (share) {
        clf->weights = share->weights;          // (nothing is copied: the table is read where it lies)
        d.w = share->d.w;
    } else {
        d.w = cls_alloc<int32_t>(clf, h, N * d.H * (size_t)d.w_stride);
        if (d.w) {                              // (the block leaves the object's own list: the last holder frees it)
            clf->allocs.pop_back();
            const int device = clf->device;
            clf->weights = std::shared_ptr<void>((void *)d.w, [device](void *p) { hipSetDevice(device); hipFree(p); });
        }
    }
    d.ring = cls_alloc<ClsPair>(clf, h, N * d.ring_len * d.max_pairs);
    d.count = cls_alloc<int64_t>(clf, h, N + 1);
    d.acc = cls_alloc<int64_t>(clf, h, N * d.H * 2 * d.B_pad);
    d.ticket = cls_alloc<uint32_t>(clf, h, std::max<size_t>(N * d.H, HTM_CLASSIFIER_MAX_HORIZONS));
    d.delta = cls_alloc<int32_t>(clf, h, N * d.H * d.B_pad);
    d.learn = cls_alloc<int32_t>(clf, h, std::max<size_t>(N * d.H, HTM_CLASSIFIER_MAX_HORIZONS));
    int32_t *table = cls_alloc<int32_t>(clf, h, HTM_CLASSIFIER_EXP);
    d.exp_table = table;
    ok = d.w && d.ring && d.count && d.acc && d.ticket && d.delta && d.learn && table;
    if (n > 1) {
        clf->d_tab = cls_alloc<void *>(clf, h, 3 * N);
        clf->d_flags = cls_alloc<int32_t>(clf, h, N);
        ok = ok && clf->d_tab && clf->d_flags;
    }
    // an empty ring holds (-1, 0) pairs; the state and the table are there when the call returns, whatever stream the first update comes on
    std::vector<ClsPair> empty(N * d.ring_len * d.max_pairs, ClsPair{-1, 0u});
    ok = ok && hipMemcpyAsync(d.ring, empty.data(), N * clf->ring_bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
         hipMemcpyAsync(table, exp_table2049, HTM_CLASSIFIER_EXP * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) == hipSuccess &&
         hipStreamSynchronize(h->stream) == hipSuccess;
    if (!ok) {
        htm_classifier_destroy(clf);
        return cls_refuse(h, what + ": device allocation failed", HTM_ERR_HIP);
    }
    *out = clf;
    return HTM_OK;
}

extern "C" int htm_classifier_create(htm_handle *h, const htm_classifier_config *cfg, const int32_t *exp_table2049, htm_classifier **out) {
    return cls_create("htm_classifier_create", h, cfg, exp_table2049, 1, nullptr, out);
}

extern "C" int htm_classifiers_create(htm_handle *h, const htm_classifier_config *cfg, const int32_t *exp_table2049, int32_t n_streams,
                                      htm_classifier *share_weights_of, htm_classifier **out) {
    return cls_create("htm_classifiers_create", h, cfg, exp_table2049, n_streams, share_weights_of, out);
}

// what every call on an existing object checks of its handle
static int cls_check(const char *what, htm_classifier *clf, htm_handle *h) {
    if (!clf || !h) return cls_refuse(h, std::string(what) + ": null argument", HTM_ERR_ARGUMENT);
    if (h->world > 1) return cls_refuse(h, std::string(what) + ": not available on a column-sharded handle", HTM_ERR_STATE);
    if (h->device != clf->device) return cls_refuse(h, std::string(what) + ": the handle is on another device than the classifier", HTM_ERR_ARGUMENT);
    return 0;
}

// ... and what the calls of a one-stream object check besides: a bank has calls of its own (htm_classifiers_*)
static int cls_check_single(const char *what, htm_classifier *clf, htm_handle *h) {
    if (int rc = cls_check(what, clf, h)) return rc;
    if (clf->n > 1) return cls_refuse(h, std::string(what) + ": the object has " + std::to_string(clf->n) + " streams: use the htm_classifiers_ calls", HTM_ERR_ARGUMENT);
    return 0;
}

// blocks along x of the launches that split a pattern of n pairs
static int cls_blocks(int n_pairs) { return (n_pairs + HTM_CLASSIFIER_PAIRS - 1) / HTM_CLASSIFIER_PAIRS; }

// The accumulators of a frozen call, for `rows` block rows (streams x steps of one launch x horizons): [rows][B_pad] sums and [rows]
// tickets, zero between launches.  Sized by what the calls ask for -- a bank that only ticks needs one step's -- and made anew when a
// call needs more (hipFree waits for the device: nothing enqueued still uses the old ones).
static int cls_frozen_rows(const char *what, htm_classifier *clf, htm_handle *h, size_t rows) {
    if (rows <= clf->frozen_rows) return 0;
    for (void *p : {(void *)clf->frozen.acc, (void *)clf->frozen.ticket}) {
        if (!p) continue;
        clf->allocs.erase(std::remove(clf->allocs.begin(), clf->allocs.end(), p), clf->allocs.end());
        hipFree(p);
    }
    clf->frozen = ClsFrozen{};
    clf->frozen_rows = 0;
    ClsFrozen f;
    f.acc = cls_alloc<int64_t>(clf, h, rows * clf->d.B_pad);
    f.ticket = cls_alloc<uint32_t>(clf, h, rows);
    if (!f.acc || !f.ticket) return cls_refuse(h, std::string(what) + ": device allocation failed", HTM_ERR_HIP);
    clf->frozen = f;
    clf->frozen_rows = rows;
    return 0;
}

// Every call below is written once, over the n streams of the object (DESIGN.md sections 24 and 25); the htm_classifier_ and
// htm_classifiers_ entry points are two doors to it.  `what` names the function that was called, `bank` its door: the one-stream door
// takes only objects of n = 1 and launches the kcls_ kernels, the bank's launches the kgcls_ kernels, at n = 1 as well.  The total is
// the object's: every call advances all streams by the same steps.
static int cls_door(const char *what, bool bank, htm_classifier *clf, htm_handle *h) { return bank ? cls_check(what, clf, h) : cls_check_single(what, clf, h); }

static GClsDev gcls_of(const htm_classifier *clf) { return GClsDev{clf->d, clf->n, clf->shares ? 0 : (int64_t)clf->d.H * clf->d.w_stride}; }

// the accumulators of a frozen call of n_steps steps: for the steps of its largest launch; through the one-stream door for a whole chunk
static int cls_prepare(htm_classifier *clf, htm_handle *h, int32_t learn, int32_t n_steps, bool bank = true) {
    const ClsDev &d = clf->d;
    if (learn) return 0;
    const size_t steps = bank ? std::min<int>(gcls_chunk(clf->n, d.H), std::max(n_steps, 1)) : HTM_CLASSIFIER_CHUNK;
    return cls_frozen_rows(bank ? "htm_classifiers_update" : "htm_classifier_update", clf, h, (size_t)clf->n * steps * d.H);
}

// The launches of an update over every stream, enqueued on stream s: 2 per step when learning, one per gcls_chunk steps otherwise.
// gs holds the call's inputs (a table in device memory, or member 0's pointers and strides); the caller has checked them.
static int cls_enqueue(htm_classifier *clf, htm_handle *h, hipStream_t s, GClsStep gs, int32_t learn, bool bank = true) {
    const ClsDev &d = clf->d;
    const int chunk = gcls_chunk(clf->n, d.H);      // (one stream: HTM_CLASSIFIER_CHUNK)
    if (int rc = cls_prepare(clf, h, learn, gs.n_steps, bank)) return rc;
    gs.total = clf->total;
    const GClsDev gd = gcls_of(clf);
    const ClsStep one{gs.pairs, gs.pairs_per_step, gs.targets, gs.reset_bits, gs.n_targets, gs.first_step, gs.best, gs.dist, gs.total};
    if (learn) {
        const dim3 grid(cls_blocks(d.max_pairs), clf->n * d.H);
        for (int i = 0; i < gs.n_steps; ++i) {
            if (bank) {
                LAUNCH_ON(h, s, 0, "classifiers:sum", kgcls_sum, grid, HTM_CLASSIFIER_THREADS, gd, gs, i);
                LAUNCH_ON(h, s, 0, "classifiers:apply", kgcls_apply, grid, HTM_CLASSIFIER_THREADS, gd, gs, i);
            } else {
                LAUNCH_ON(h, s, 0, "classifier:sum", kcls_sum, grid, HTM_CLASSIFIER_THREADS, d, one, i);
                LAUNCH_ON(h, s, 0, "classifier:apply", kcls_apply, grid, HTM_CLASSIFIER_THREADS, d, one, i);
            }
        }
    } else {
        for (int first = 0; first < gs.n_steps; first += chunk) {
            const int n = std::min<int>(chunk, gs.n_steps - first);
            const dim3 grid(cls_blocks(gs.pairs_per_step), clf->n * n * d.H);
            if (bank) LAUNCH_ON(h, s, 0, "classifiers:frozen", kgcls_frozen, grid, HTM_CLASSIFIER_THREADS, gd, clf->frozen, gs, first, n);
            else LAUNCH_ON(h, s, 0, "classifier:frozen", kcls_frozen, grid, HTM_CLASSIFIER_THREADS, d, clf->frozen, one, first, n);
        }
    }
    clf->total += gs.n_steps;
    return 0;
}

// the inputs per stream: tables of n device pointers (reset bits: or null)
static int cls_update(const char *what, bool bank, htm_classifier *clf, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                      const int32_t *const *device_targets, int32_t n_targets, int32_t first_step, const uint32_t *const *device_reset_bits, int32_t learn,
                      int32_t *device_best, int32_t *device_dist) {
    if (int rc = cls_door(what, bank, clf, h)) return rc;
    const std::string w = std::string(what) + ": ";
    if (!device_pairs || !device_targets || !device_best) return cls_refuse(h, w + "null pairs, targets or output", HTM_ERR_ARGUMENT);
    const ClsDev &d = clf->d;
    const size_t n = (size_t)clf->n;
    for (size_t i = 0; i < n; ++i)
        if (!device_pairs[i] || !device_targets[i] || (device_reset_bits && !device_reset_bits[i]))
            return cls_refuse(h, w + "stream " + std::to_string(i) + " has no pairs, targets or reset bits", HTM_ERR_ARGUMENT);
    if (pairs_per_step < 1 || pairs_per_step > d.max_pairs)
        return cls_refuse(h, w + "pairs_per_step must be in [1, max_pairs = " + std::to_string(d.max_pairs) + "]", HTM_ERR_ARGUMENT);
    if (n_steps < 0 || n_targets < 1 || first_step < 0) return cls_refuse(h, w + "n_steps >= 0, n_targets >= 1, first_step >= 0", HTM_ERR_ARGUMENT);
    // (an empty call that would learn on another object's table: refused through the bank's door, nothing through the one-stream door)
    if (learn && clf->shares && (bank || n_steps > 0)) return cls_refuse(h, w + "the streams read another object's weight table: learn must be 0", HTM_ERR_STATE);
    if (n_steps == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(clf->device));
    GClsStep gs{};
    if (n > 1) {
        // the one copy of the pointer table, from the call's own (pageable) words: the copy has read them when it returns (htm_likelihood_update)
        std::vector<const void *> tab(3 * n, nullptr);
        for (size_t i = 0; i < n; ++i) {
            tab[i] = device_pairs[i];
            tab[n + i] = device_targets[i];
            if (device_reset_bits) tab[2 * n + i] = device_reset_bits[i];
        }
        HIPCHK(h, hipMemcpyAsync((void *)clf->d_tab, (const void *)tab.data(), 3 * n * sizeof(void *), hipMemcpyHostToDevice, h->stream));
        gs.pairs_tab = (const ClsPair *const *)clf->d_tab;
        gs.targets_tab = (const int32_t *const *)(clf->d_tab + n);
        gs.resets_tab = device_reset_bits ? (const uint32_t *const *)(clf->d_tab + 2 * n) : nullptr;
    } else {
        gs.pairs = (const ClsPair *)device_pairs[0];
        gs.targets = device_targets[0];
        gs.reset_bits = device_reset_bits ? device_reset_bits[0] : nullptr;
    }
    gs.pairs_per_step = pairs_per_step; gs.n_targets = n_targets; gs.first_step = first_step; gs.n_steps = n_steps;
    gs.best = device_best; gs.dist = device_dist;
    if (int rc = cls_enqueue(clf, h, h->stream, gs, learn, bank)) return rc;
    return launch_status(h->err);
}

extern "C" int htm_classifier_update(htm_classifier *clf, htm_handle *h, const void *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                                     const int32_t *device_targets, int32_t n_targets, int32_t first_step, const uint32_t *device_reset_bits,
                                     int32_t learn, int32_t *device_best, int32_t *device_dist) {
    return cls_update("htm_classifier_update", false, clf, h, &device_pairs, pairs_per_step, n_steps, &device_targets, n_targets, first_step,
                      device_reset_bits ? &device_reset_bits : nullptr, learn, device_best, device_dist);
}
extern "C" int htm_classifiers_update(htm_classifier *clf, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                                      const int32_t *const *device_targets, int32_t n_targets, int32_t first_step, const uint32_t *const *device_reset_bits,
                                      int32_t learn, int32_t *device_best, int32_t *device_dist) {
    return cls_update("htm_classifiers_update", true, clf, h, device_pairs, pairs_per_step, n_steps, device_targets, n_targets, first_step, device_reset_bits, learn,
                      device_best, device_dist);
}

// the histories of the streams that `streams` names emptied (null: every stream's)
static int cls_reset(const char *what, bool bank, htm_classifier *clf, htm_handle *h, const uint8_t *streams) {
    if (int rc = cls_door(what, bank, clf, h)) return rc;
    HIPCHK(h, hipSetDevice(clf->device));
    if (!streams || clf->n == 1) {
        if (!streams || streams[0]) HIPCHK(h, hipMemsetAsync(clf->d.count, 0, (size_t)clf->n * 8, h->stream));
        return HTM_OK;
    }
    std::vector<int32_t> flags((size_t)clf->n);     // (the call's own pageable words: the copy has read them when it returns)
    for (int i = 0; i < clf->n; ++i) flags[i] = streams[i] ? 1 : 0;
    HIPCHK(h, hipMemcpyAsync(clf->d_flags, flags.data(), flags.size() * 4, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "classifiers:reset", kgcls_reset, (clf->n + 255) / 256, 256, clf->d.count, (const int32_t *)clf->d_flags, clf->n);
    return launch_status(h->err);
}

extern "C" int htm_classifier_reset(htm_classifier *clf, htm_handle *h) { return cls_reset("htm_classifier_reset", false, clf, h, nullptr); }
extern "C" int htm_classifiers_reset(htm_classifier *clf, htm_handle *h, const uint8_t *streams) { return cls_reset("htm_classifiers_reset", true, clf, h, streams); }

// The rows [unit0, unit0 + n_units) of one stream's, one horizon's table copied to the host (write == 0) or from it; host rows are B
// words, device rows B_pad.  (The padding buckets of a row stay 0: nothing ever writes them.)
static int cls_weights(const char *what, bool bank, bool write, htm_classifier *clf, htm_handle *h, int32_t stream, int32_t horizon, int32_t unit0, int32_t n_units,
                       int32_t *host) {
    if (int rc = cls_door(what, bank, clf, h)) return rc;
    const ClsDev &d = clf->d;
    const int64_t units = d.w_stride / d.B_pad;
    if (!host || stream < 0 || stream >= clf->n || horizon < 0 || horizon >= d.H || unit0 < 0 || n_units < 0 || (int64_t)unit0 + n_units > units)
        return cls_refuse(h, std::string(what) + ": need host memory, a stream below n_streams, a horizon index below n_steps and rows inside the table", HTM_ERR_ARGUMENT);
    if (write && clf->shares) return cls_refuse(h, std::string(what) + ": the object reads another object's weights: write them there", HTM_ERR_STATE);
    for (size_t i = 0; write && i < (size_t)n_units * d.B; ++i)
        if (host[i] > HTM_CLASSIFIER_W_LIMIT || host[i] < -HTM_CLASSIFIER_W_LIMIT)
            return cls_refuse(h, std::string(what) + ": a weight is outside [-2^30, 2^30]", HTM_ERR_ARGUMENT);
    if (n_units == 0) return HTM_OK;
    int32_t *rows = d.w + (int64_t)stream * gcls_of(clf).w_member + (int64_t)horizon * d.w_stride + (int64_t)unit0 * d.B_pad;
    const size_t host_pitch = (size_t)d.B * 4, dev_pitch = (size_t)d.B_pad * 4;
    HIPCHK(h, hipSetDevice(clf->device));
    if (write) HIPCHK(h, hipMemcpy2DAsync(rows, dev_pitch, host, host_pitch, host_pitch, (size_t)n_units, hipMemcpyHostToDevice, h->stream));
    else HIPCHK(h, hipMemcpy2DAsync(host, host_pitch, rows, dev_pitch, host_pitch, (size_t)n_units, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return HTM_OK;
}

extern "C" int htm_classifier_read_weights(htm_classifier *clf, htm_handle *h, int32_t horizon, int32_t unit0, int32_t n_units, int32_t *host_dst) {
    return cls_weights("htm_classifier_read_weights", false, false, clf, h, 0, horizon, unit0, n_units, host_dst);
}
extern "C" int htm_classifier_write_weights(htm_classifier *clf, htm_handle *h, int32_t horizon, int32_t unit0, int32_t n_units, const int32_t *host_src) {
    return cls_weights("htm_classifier_write_weights", false, true, clf, h, 0, horizon, unit0, n_units, (int32_t *)host_src);
}
extern "C" int htm_classifiers_read_weights(htm_classifier *clf, htm_handle *h, int32_t stream, int32_t horizon, int32_t unit0, int32_t n_units, int32_t *host_dst) {
    return cls_weights("htm_classifiers_read_weights", true, false, clf, h, stream, horizon, unit0, n_units, host_dst);
}
extern "C" int htm_classifiers_write_weights(htm_classifier *clf, htm_handle *h, int32_t stream, int32_t horizon, int32_t unit0, int32_t n_units, const int32_t *host_src) {
    return cls_weights("htm_classifiers_write_weights", true, true, clf, h, stream, horizon, unit0, n_units, (int32_t *)host_src);
}

// The state of n streams: int64 total; int64 count[n]; the rings [n][ring_len][max_pairs] -- at n = 1 the (total, count, ring) of the
// one-stream door.  The size calls have no handle to refuse through: the one-stream one gives one stream's size for any object.
static int64_t cls_state_bytes(const htm_classifier *clf, size_t n) { return clf ? (int64_t)(8 + n * 8 + n * clf->ring_bytes) : (int64_t)HTM_ERR_ARGUMENT; }

extern "C" int64_t htm_classifier_state_bytes(const htm_classifier *clf) { return cls_state_bytes(clf, 1); }
extern "C" int64_t htm_classifiers_state_bytes(const htm_classifier *clf) { return cls_state_bytes(clf, clf ? (size_t)clf->n : 1); }

// the state copied to the host blob (load == 0) or from it, behind everything enqueued on h's stream
static int cls_state(const char *what, bool bank, bool load, htm_classifier *clf, htm_handle *h, void *host_state, int64_t bytes) {
    if (int rc = cls_door(what, bank, clf, h)) return rc;
    const size_t n = (size_t)clf->n;
    if (!host_state || bytes != cls_state_bytes(clf, n)) return cls_refuse(h, std::string(what) + ": need host_state of the state_bytes call's bytes", HTM_ERR_ARGUMENT);
    char *ring = (char *)host_state + (n + 1) * 8;
    std::vector<int64_t> head(n + 1);               // total, count[n]
    if (load) memcpy(head.data(), host_state, (n + 1) * 8);
    for (size_t i = 1; load && i <= n; ++i)         // (a learning step looks count steps back in the ring: never before step 0)
        if (head[i] < 0 || head[i] > head[0])
            return cls_refuse(h, std::string(what) + ": need 0 <= count <= total in stream " + std::to_string(i - 1), HTM_ERR_ARGUMENT);
    HIPCHK(h, hipSetDevice(clf->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (load) {
        HIPCHK(h, hipMemcpy(clf->d.count, head.data() + 1, n * 8, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(clf->d.ring, ring, n * clf->ring_bytes, hipMemcpyHostToDevice));
        clf->total = head[0];
    } else {
        memcpy(host_state, &clf->total, 8);
        HIPCHK(h, hipMemcpy((char *)host_state + 8, clf->d.count, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(ring, clf->d.ring, n * clf->ring_bytes, hipMemcpyDeviceToHost));
    }
    return HTM_OK;
}

extern "C" int htm_classifier_export(htm_classifier *clf, htm_handle *h, void *host_state, int64_t bytes) {
    return cls_state("htm_classifier_export", false, false, clf, h, host_state, bytes);
}
extern "C" int htm_classifier_import(htm_classifier *clf, htm_handle *h, const void *host_state, int64_t bytes) {
    return cls_state("htm_classifier_import", false, true, clf, h, (void *)host_state, bytes);
}
extern "C" int htm_classifiers_export(htm_classifier *clf, htm_handle *h, void *host_state, int64_t bytes) {
    return cls_state("htm_classifiers_export", true, false, clf, h, host_state, bytes);
}
extern "C" int htm_classifiers_import(htm_classifier *clf, htm_handle *h, const void *host_state, int64_t bytes) {
    return cls_state("htm_classifiers_import", true, true, clf, h, (void *)host_state, bytes);
}

// ------------------------------------------------------------------------------------------
// KNN classifiers (htm_knn.h, htm_knn_bank.h; DESIGN.md sections 26 and 27): the stores, their labels and stamps and the scratch of an
// update in device memory; the slots in use, the step total and the labels of the learning calls on the host -- every store is decided
// here, nothing is read back.  As the classifier it keeps nothing of the handles its calls come through.  Every host call is written
// once, as knn_<call>(what, bank, ...): `bank` is the door the call came through (htm_knns_*; false: htm_knn_*), and the one-stream
// object is the n == 1 case with the one-stream kernels.
struct htm_knn {
    int device = 0;
    KnnDev d{};
    std::vector<int32_t> counts;                // [n] the slots in use ...
    int32_t count = 0;                          // ... and the largest of them
    int64_t total = 0;
    int64_t device_bytes = 0;
    std::vector<void *> allocs;
    std::vector<int32_t> labels;                // htm_knn_labels: the labels a learning call reads, as the host gave them
    int32_t *d_labels = nullptr;                // ... and their device array, of labels_cap words
    size_t labels_cap = 0;
    int32_t *d_pos = nullptr;                   // the slot of every step of the call in flight, of pos_cap words
    size_t pos_cap = 0;
    // n streams (a one-stream object: 1): n stores member-major in d's arrays, or, in a bank, n frozen streams over `source`'s
    int32_t n = 1, chunk = HTM_KNN_CHUNK;
    int refs = 1;                               // the object itself and every bank that shares its store
    htm_knn *source = nullptr;
    void **d_tab = nullptr;                     // a bank's [n] input pointers, then [n][2] counts: the table of the update in flight
    bool is_bank = false;
};

extern "C" void htm_knn_destroy(htm_knn *knn) {
    if (!knn || --knn->refs > 0) return;        // (a store that banks still read lives until the last of them goes)
    hipSetDevice(knn->device);
    for (void *p : knn->allocs) hipFree(p);     // (hipFree waits for the device: nothing enqueued still reads them)
    htm_knn *source = knn->source;
    delete knn;
    htm_knn_destroy(source);
}

// zeroed device memory of the object's, ordered on h's stream (null: the allocation failed)
template <typename T>
static T *knn_alloc(htm_knn *knn, htm_handle *h, size_t count) {
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    knn->allocs.push_back(p);
    knn->device_bytes += (int64_t)bytes;
    if (hipMemsetAsync(p, 0, bytes, h->stream) != hipSuccess) return nullptr;
    return (T *)p;
}

// a scratch array of the object's grown to `count` words (hipFree waits for the device: nothing enqueued still uses the old one)
static int knn_grow(const char *what, htm_knn *knn, htm_handle *h, int32_t **p, size_t *cap, size_t count) {
    if (count <= *cap) return 0;
    if (*p) {
        knn->allocs.erase(std::remove(knn->allocs.begin(), knn->allocs.end(), (void *)*p), knn->allocs.end());
        knn->device_bytes -= (int64_t)(*cap * 4);
        hipFree(*p);
        *p = nullptr;
        *cap = 0;
    }
    count = std::max<size_t>(count, 256);
    int32_t *q = knn_alloc<int32_t>(knn, h, count);
    if (!q) return cls_refuse(h, std::string(what) + ": device allocation failed", HTM_ERR_HIP);
    *p = q;
    *cap = count;
    return 0;
}

// what a create call checks of its handle and its config (and of n_streams, where a bank's checks have it), and the scalar fields of
// the KnnDev the config asks for; *words: the words of one query's table, not yet narrowed
static int knn_config(const std::string &what, htm_handle *h, const htm_knn_config *cfg, int32_t n_streams, KnnDev *dev, int64_t *words) {
    if (cfg->struct_bytes != sizeof(htm_knn_config)) return cls_refuse(h, what + ": htm_knn_config size mismatch", HTM_ERR_ARGUMENT);
    const bool ok = cfg->labels >= 1 && cfg->labels <= HTM_KNN_MAX_LABELS && cfg->k >= 1 && cfg->k <= HTM_KNN_MAX_K && cfg->min_overlap >= 1 &&
                    cfg->min_overlap <= 65535 && cfg->capacity >= 1 && cfg->capacity <= HTM_KNN_MAX_CAPACITY && cfg->cell_dim >= 1 && cfg->cell_dim <= 64 &&
                    cfg->units >= cfg->cell_dim && cfg->units % cfg->cell_dim == 0 && cfg->max_pairs >= 1 && cfg->max_pairs <= HTM_KNN_MAX_PAIRS;
    if (!ok)
        return cls_refuse(h, what + ": labels in [1, 1024], k in [1, 64], min_overlap in [1, 65535], capacity in [1, 2^20], cell_dim in [1, 64], "
                             "units a positive multiple of cell_dim, max_pairs in [1, 2047]", HTM_ERR_ARGUMENT);
    if (n_streams < 1 || n_streams > HTM_KNNS_MAX_STREAMS) return cls_refuse(h, what + ": n_streams must be in [1, 65535]", HTM_ERR_ARGUMENT);
    if (h->world > 1) return cls_refuse(h, what + ": not available on a column-sharded handle", HTM_ERR_STATE);
    KnnDev d{};
    d.labels = cfg->labels;
    d.k = cfg->k;
    d.min_overlap = cfg->min_overlap;
    d.capacity = cfg->capacity;
    d.K = cfg->cell_dim;
    d.WPC = (cfg->cell_dim + 31) / 32;
    d.n_cols = cfg->units / cfg->cell_dim;
    d.max_pairs = cfg->max_pairs;
    *words = knn_table_words(d.n_cols, d.WPC);
    d.words = (int32_t)*words;
    d.queries = knn_queries(*words);
    d.in_lds = knn_in_lds(*words);
    d.bitmap = knn_has_bitmap(*words);
    d.shift = knn_shift(knn_max_overlap(d.max_pairs, d.K));
    *dev = d;
    return 0;
}

// A one-stream object (bank == false: n_streams 1, chunks of HTM_KNN_CHUNK, no table of an update), a bank of n_streams stores, or a
// bank of n_streams frozen streams over the store of `share`: that one holds scratch only.
static int knn_create(const std::string &what, bool bank, htm_handle *h, const htm_knn_config *cfg, int32_t n_streams, htm_knn *share, htm_knn **out) {
    if (out) *out = nullptr;
    if (!h || !cfg || !out) return cls_refuse(h, what + ": null argument", HTM_ERR_ARGUMENT);
    KnnDev d{};
    int64_t words = 0;
    if (int rc = knn_config(what, h, cfg, n_streams, &d, &words)) return rc;
    if (share) {
        if (share->is_bank) return cls_refuse(h, what + ": share_store_of is a bank: only a one-stream object's store is shared", HTM_ERR_ARGUMENT);
        if (share->device != h->device) return cls_refuse(h, what + ": share_store_of is on another device than the handle", HTM_ERR_ARGUMENT);
        const KnnDev &sd = share->d;
        if (sd.labels != d.labels || sd.k != d.k || sd.min_overlap != d.min_overlap || sd.capacity != d.capacity || sd.K != d.K || sd.n_cols != d.n_cols ||
            sd.max_pairs != d.max_pairs)
            return cls_refuse(h, what + ": share_store_of was made with another config", HTM_ERR_ARGUMENT);
        d.store = sd.store; d.label = sd.label; d.stamp = sd.stamp;     // (where they lie; the scratch is the bank's own)
    }
    // (the streams of a shared store are one flat batch of queries: a chunk that takes a tick's n queries in one launch where that fits)
    const int chunk = !bank ? HTM_KNN_CHUNK : share ? gknn_shared_chunk(n_streams, d.capacity, words) : gknn_chunk(n_streams, d.capacity, words);
    if (bank && (words > INT32_MAX || chunk < 1))
        return cls_refuse(h, what + ": the scratch of one query step of " + std::to_string(n_streams) + " streams does not fit " +
                                 std::to_string(HTM_KNNS_SCRATCH_BYTES >> 20) + " MiB: fewer streams or a smaller capacity", HTM_ERR_ARGUMENT);
    HIPCHK(h, hipSetDevice(h->device));
    htm_knn *knn = new htm_knn();
    knn->device = h->device;
    knn->is_bank = bank;
    knn->n = n_streams;
    knn->chunk = chunk;
    knn->counts.assign((size_t)n_streams, 0);
    const size_t cap = (size_t)d.capacity, n = (size_t)n_streams, rows = (share ? 1 : n) * (size_t)chunk;
    if (!share) {
        d.store = knn_alloc<ClsPair>(knn, h, n * cap * d.max_pairs);
        d.label = knn_alloc<int32_t>(knn, h, n * cap);
        d.stamp = knn_alloc<int64_t>(knn, h, n * cap);
    }
    d.ovl = knn_alloc<uint16_t>(knn, h, rows * cap);
    d.table = d.in_lds ? nullptr : knn_alloc<uint32_t>(knn, h, rows * (size_t)words);
    if (bank && !share) knn->d_tab = knn_alloc<void *>(knn, h, 2 * n);      // (n pointers and n x 2 counts of 4 bytes)
    knn->d = d;
    // (the state is there when the call returns, whatever stream the first update comes on)
    if (words > INT32_MAX || !d.store || !d.label || !d.stamp || !d.ovl || (!d.in_lds && !d.table) || (bank && !share && !knn->d_tab) ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
        htm_knn_destroy(knn);
        return cls_refuse(h, what + ": device allocation failed", HTM_ERR_HIP);
    }
    if (share) {
        knn->source = share;
        ++share->refs;
    }
    *out = knn;
    return HTM_OK;
}

extern "C" int htm_knn_create(htm_handle *h, const htm_knn_config *cfg, htm_knn **out) { return knn_create("htm_knn_create", false, h, cfg, 1, nullptr, out); }
extern "C" int htm_knns_create(htm_handle *h, const htm_knn_config *cfg, int32_t n_streams, htm_knn *share_store_of, htm_knn **out) {
    return knn_create("htm_knns_create", true, h, cfg, n_streams, share_store_of, out);
}

// what every call on an existing object checks of its handle
static int knn_check(const char *what, htm_knn *knn, htm_handle *h, bool bank = false) {
    if (!knn || !h) return cls_refuse(h, std::string(what) + ": null argument", HTM_ERR_ARGUMENT);
    if (h->world > 1) return cls_refuse(h, std::string(what) + ": not available on a column-sharded handle", HTM_ERR_STATE);
    if (h->device != knn->device) return cls_refuse(h, std::string(what) + ": the handle is on another device than the KNN classifier", HTM_ERR_ARGUMENT);
    if (!bank && knn->is_bank) return cls_refuse(h, std::string(what) + ": the object is a bank of streams: use the htm_knns_ calls", HTM_ERR_STATE);
    if (bank && !knn->is_bank) return cls_refuse(h, std::string(what) + ": the object is a one-stream KNN classifier: use the htm_knn_ calls", HTM_ERR_STATE);
    return 0;
}

// host labels [n][n_labels] into the object's own array
static int knn_labels(const char *what, bool bank, htm_knn *knn, htm_handle *h, const int32_t *host_labels, int32_t n_labels, const int32_t **device_labels) {
    if (device_labels) *device_labels = nullptr;
    if (int rc = knn_check(what, knn, h, bank)) return rc;
    if (!host_labels || !device_labels || n_labels < 1) return cls_refuse(h, std::string(what) + ": need host labels, n_labels >= 1 and a place for the address", HTM_ERR_ARGUMENT);
    const size_t words = (size_t)knn->n * (size_t)n_labels;
    HIPCHK(h, hipSetDevice(knn->device));
    if (int rc = knn_grow(what, knn, h, &knn->d_labels, &knn->labels_cap, words)) return rc;
    knn->labels.assign(host_labels, host_labels + words);
    // (from the call's own pageable words: the copy has read them when it returns)
    HIPCHK(h, hipMemcpyAsync(knn->d_labels, host_labels, words * 4, hipMemcpyHostToDevice, h->stream));
    *device_labels = knn->d_labels;
    return HTM_OK;
}

extern "C" int htm_knn_labels(htm_knn *knn, htm_handle *h, const int32_t *host_labels, int32_t n_labels, const int32_t **device_labels) {
    return knn_labels("htm_knn_labels", false, knn, h, host_labels, n_labels, device_labels);
}
extern "C" int htm_knns_labels(htm_knn *knn, htm_handle *h, const int32_t *host_labels, int32_t n_labels, const int32_t **device_labels) {
    return knn_labels("htm_knns_labels", true, knn, h, host_labels, n_labels, device_labels);
}

// the launches of the queries [0, s.n_steps) of one flat batch against a one-stream view (d, s) in chunks, profiled as knn:... for a
// one-stream object's call and as knns:... for a sharing bank's
#define KNN_NAME(bank, tail) ((bank) ? "knns:" tail : "knn:" tail)
static int knn_enqueue_queries(htm_handle *h, hipStream_t st, bool bank, const KnnDev &d, const KnnStep &s, int chunk) {
    for (int first = 0; first < s.n_steps; first += chunk) {
        const int nq = std::min<int>(chunk, s.n_steps - first);
        const unsigned scatter = (unsigned)(((int64_t)nq * s.pairs_per_step + 255) / 256);
        if (s.count > 0) {
            const dim3 grid(knn_slot_blocks(s.count), knn_query_groups(nq, d.queries));
            if (d.in_lds) {
                LAUNCH_ON(h, st, (size_t)knn_distance_lds(d.words), KNN_NAME(bank, "distance"), kknn_distance_lds, grid, 256, d, s, first, nq);
            } else {
                LAUNCH_ON(h, st, 0, KNN_NAME(bank, "scatter"), kknn_scatter, scatter, 256, d, s, first, nq, 1);
                LAUNCH_ON(h, st, (size_t)knn_distance_lds(d.words), KNN_NAME(bank, "distance"), kknn_distance_global, grid, 256, d, s, first, nq);
            }
        }
        LAUNCH_ON(h, st, 0, KNN_NAME(bank, "select"), kknn_select, nq, 256, d, s, first);
        if (s.count > 0 && !d.in_lds) LAUNCH_ON(h, st, 0, KNN_NAME(bank, "clear"), kknn_scatter, scatter, 256, d, s, first, nq, 0);
    }
    return 0;
}

// The launches of an update of a bank's own stores, enqueued on stream st: gs holds the call's inputs, `largest` the largest count
// behind the call's append, `stores` whether any stream stores; `place`: the slots come from kgknn_place (a tick's come with gs.pos).
static int knns_enqueue(htm_knn *knn, htm_handle *h, hipStream_t st, const GKnnStep &gs, int32_t largest, bool stores, bool place) {
    const KnnDev &d = knn->d;
    const GKnnDev g{d, knn->n, knn->chunk};
    const int n_steps = gs.s.n_steps, pairs_per_step = gs.s.pairs_per_step;
    if (stores) {
        if (place) LAUNCH_ON(h, st, 0, "knns:place", kgknn_place, knn->n, 256, g, gs);
        LAUNCH_ON(h, st, 0, "knns:append", kgknn_append, dim3((unsigned)(((int64_t)n_steps * d.max_pairs + 255) / 256), knn->n), 256, g, gs);
    }
    for (int first = 0; first < n_steps; first += knn->chunk) {
        const int nq = std::min<int>(knn->chunk, n_steps - first);
        const dim3 scatter((unsigned)(((int64_t)nq * pairs_per_step + 255) / 256), knn->n);
        if (largest > 0) {
            const dim3 grid(knn_slot_blocks(largest), gknn_distance_rows(knn->n, nq, d.queries));
            if (d.in_lds) {
                LAUNCH_ON(h, st, (size_t)knn_distance_lds(d.words), "knns:distance", kgknn_distance_lds, grid, 256, g, gs, first, nq);
            } else {
                LAUNCH_ON(h, st, 0, "knns:scatter", kgknn_scatter, scatter, 256, g, gs, first, nq, 1);
                LAUNCH_ON(h, st, (size_t)knn_distance_lds(d.words), "knns:distance", kgknn_distance_global, grid, 256, g, gs, first, nq);
            }
        }
        LAUNCH_ON(h, st, 0, "knns:select", kgknn_select, dim3(nq, knn->n), 256, g, gs, first);
        if (largest > 0 && !d.in_lds) LAUNCH_ON(h, st, 0, "knns:clear", kgknn_scatter, scatter, 256, g, gs, first, nq, 0);
    }
    return 0;
}

// the n x n_steps frozen queries of a sharing bank, one flat batch over the source's store as it is now: every slot in [0, count) is seen
static int knns_enqueue_shared(htm_knn *knn, htm_handle *h, hipStream_t st, const ClsPair *pairs, int32_t pairs_per_step, int64_t queries, int32_t *best,
                               int32_t *votes) {
    KnnDev d = knn->d;
    const KnnDev &sd = knn->source->d;
    d.store = sd.store; d.label = sd.label; d.stamp = sd.stamp;
    const int32_t count = knn->source->count;
    const KnnStep s{pairs, pairs_per_step, nullptr, 1, 0, (int32_t)queries, best, votes, INT64_MAX / 2, count, count};
    return knn_enqueue_queries(h, st, true, d, s, knn->chunk);
}

// the steps of [first_step, first_step + n_steps) that stream m stores: counted on the host, from the labels the host gave
static int64_t knn_stored(const htm_knn *knn, size_t m, int32_t first_step, int32_t n_steps, int32_t n_labels) {
    int64_t stored = 0;
    for (int i = 0; i < n_steps; ++i) {
        const int32_t g = knn->labels[m * (size_t)n_labels + (size_t)(((int64_t)first_step + i) % n_labels)];
        stored += g >= 0 && g < knn->d.labels;
    }
    return stored;
}

// the refusal of a call that would take stream m past its capacity (the stream is named through the bank's door)
static int knn_refuse_full(htm_handle *h, const std::string &w, bool bank, size_t m, int64_t stored, int32_t count, int32_t capacity) {
    return cls_refuse(h, w + (bank ? "stream " + std::to_string(m) + ": " : "") + "the call would store " + std::to_string(stored) + " patterns in a store of " +
                             std::to_string(count) + " of capacity = " + std::to_string(capacity) + " slots", HTM_ERR_CAPACITY);
}

// One update of every stream over n_steps steps' patterns: device_pairs holds the streams' n addresses.  A one-stream object always
// needs its labels; a bank only to learn.
static int knn_update(const char *what, bool bank, htm_knn *knn, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                      const int32_t *device_labels, int32_t n_labels, int32_t first_step, int32_t learn, int32_t *device_best, int32_t *device_votes) {
    if (int rc = knn_check(what, knn, h, bank)) return rc;
    const std::string w = std::string(what) + ": ";
    if (!device_pairs || (!bank && !device_pairs[0]) || !device_best || ((learn || !bank) && !device_labels))
        return cls_refuse(h, w + "null pairs, labels or output", HTM_ERR_ARGUMENT);
    const size_t n = (size_t)knn->n;
    for (size_t i = 0; i < n; ++i)
        if (!device_pairs[i]) return cls_refuse(h, w + "stream " + std::to_string(i) + " has no pairs", HTM_ERR_ARGUMENT);
    const KnnDev &d = knn->d;
    if (pairs_per_step < 1 || pairs_per_step > d.max_pairs)
        return cls_refuse(h, w + "pairs_per_step must be in [1, max_pairs = " + std::to_string(d.max_pairs) + "]", HTM_ERR_ARGUMENT);
    if (n_steps < 0 || n_labels < 1 || first_step < 0) return cls_refuse(h, w + "n_steps >= 0, n_labels >= 1, first_step >= 0", HTM_ERR_ARGUMENT);
    if (learn && knn->source) return cls_refuse(h, w + "the streams read another object's store: learn must be 0", HTM_ERR_STATE);
    if (bank && (int64_t)n * n_steps > INT32_MAX / 8) return cls_refuse(h, w + "n_streams x n_steps must stay below 2^28", HTM_ERR_ARGUMENT);
    // what every stream stores; one stream past its capacity refuses the call
    std::vector<int32_t> after(knn->counts);
    int64_t stored_all = 0;
    if (learn && n_steps > 0) {
        if (device_labels != knn->d_labels || (size_t)n_labels * n != knn->labels.size())
            return cls_refuse(h, w + "a learning call reads the labels of " + (bank ? "htm_knns_labels" : "htm_knn_labels") +
                                     " (its address, its n_labels): the host counts what is stored", HTM_ERR_ARGUMENT);
        for (size_t m = 0; m < n; ++m) {
            const int64_t stored = knn_stored(knn, m, first_step, n_steps, n_labels);
            if (knn->counts[m] + stored > d.capacity) return knn_refuse_full(h, w, bank, m, stored, knn->counts[m], d.capacity);
            after[m] += (int32_t)stored;
            stored_all += stored;
        }
    }
    if (n_steps == 0) return HTM_OK;
    HIPCHK(h, hipSetDevice(knn->device));
    const hipStream_t st = h->stream;
    if (knn->source) {
        // one flat batch of n x n_steps frozen queries over the source's store as it is now: every slot in [0, count) is seen
        const char *first_row = (const char *)device_pairs[0];
        const size_t row_bytes = (size_t)n_steps * pairs_per_step * sizeof(ClsPair);
        for (size_t i = 1; i < n; ++i)
            if ((const char *)device_pairs[i] != first_row + i * row_bytes)
                return cls_refuse(h, w + "the streams of a shared store are one batch: their pairs must lie one behind the other in stream order", HTM_ERR_ARGUMENT);
        if (int rc = knns_enqueue_shared(knn, h, st, (const ClsPair *)device_pairs[0], pairs_per_step, (int64_t)n * n_steps, device_best, device_votes)) return rc;
        knn->total += n_steps;
        return launch_status(h->err);
    }
    if (stored_all)
        if (int rc = knn_grow(what, knn, h, &knn->d_pos, &knn->pos_cap, n * (size_t)n_steps)) return rc;
    int32_t largest = 0;
    for (int32_t c : after) largest = std::max(largest, c);
    if (!bank) {
        // the one-stream kernels over the object's own store
        const KnnStep s{(const ClsPair *)device_pairs[0], pairs_per_step, device_labels, n_labels, first_step, n_steps, device_best, device_votes, knn->total,
                        knn->counts[0], after[0]};
        if (stored_all) {
            LAUNCH_ON(h, st, 0, "knn:place", kknn_place, 1, 256, d, s, knn->d_pos);
            LAUNCH_ON(h, st, 0, "knn:append", kknn_append, (unsigned)(((int64_t)n_steps * d.max_pairs + 255) / 256), 256, d, s, (const int32_t *)knn->d_pos);
        }
        if (int rc = knn_enqueue_queries(h, st, false, d, s, knn->chunk)) return rc;
    } else {
        // the one copy of the table, from the call's own (pageable) words: the copy has read them when it returns
        std::vector<void *> tab(2 * n, nullptr);
        int32_t *tab_counts = (int32_t *)(tab.data() + n);
        for (size_t m = 0; m < n; ++m) {
            tab[m] = (void *)device_pairs[m];
            tab_counts[2 * m] = knn->counts[m];
            tab_counts[2 * m + 1] = after[m];
        }
        HIPCHK(h, hipMemcpyAsync((void *)knn->d_tab, (const void *)tab.data(), 2 * n * sizeof(void *), hipMemcpyHostToDevice, st));
        GKnnStep gs{};
        gs.s = KnnStep{nullptr, pairs_per_step, device_labels, n_labels, first_step, n_steps, device_best, device_votes, knn->total, 0, 0};
        gs.pairs = (const ClsPair *const *)knn->d_tab;
        gs.counts = (const int32_t *)(knn->d_tab + n);
        gs.pos = stored_all ? knn->d_pos : nullptr;
        if (int rc = knns_enqueue(knn, h, st, gs, largest, stored_all > 0, true)) return rc;
    }
    knn->counts.swap(after);
    knn->count = largest;
    knn->total += n_steps;
    return launch_status(h->err);
}

extern "C" int htm_knn_update(htm_knn *knn, htm_handle *h, const void *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                              const int32_t *device_labels, int32_t n_labels, int32_t first_step, int32_t learn, int32_t *device_best,
                              int32_t *device_votes) {
    return knn_update("htm_knn_update", false, knn, h, &device_pairs, pairs_per_step, n_steps, device_labels, n_labels, first_step, learn, device_best, device_votes);
}
extern "C" int htm_knns_update(htm_knn *knn, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                               const int32_t *device_labels, int32_t n_labels, int32_t first_step, int32_t learn, int32_t *device_best,
                               int32_t *device_votes) {
    return knn_update("htm_knns_update", true, knn, h, device_pairs, pairs_per_step, n_steps, device_labels, n_labels, first_step, learn, device_best, device_votes);
}

// the stores of the streams that `streams` names emptied (null: every stream's): the slots in use are the host's (the launches enqueued
// before carry their own counts)
static int knn_reset(const char *what, bool bank, htm_knn *knn, htm_handle *h, const uint8_t *streams) {
    if (int rc = knn_check(what, knn, h, bank)) return rc;
    knn->count = 0;
    for (size_t m = 0; m < (size_t)knn->n; ++m) {
        if (!streams || streams[m]) knn->counts[m] = 0;
        knn->count = std::max(knn->count, knn->counts[m]);
    }
    return HTM_OK;
}

extern "C" int htm_knn_reset(htm_knn *knn, htm_handle *h) { return knn_reset("htm_knn_reset", false, knn, h, nullptr); }
extern "C" int htm_knns_reset(htm_knn *knn, htm_handle *h, const uint8_t *streams) { return knn_reset("htm_knns_reset", true, knn, h, streams); }

// The state: int64 total; int64 count[n]; then the streams' pairs, the streams' int64 stamps, the streams' int32 labels, each in
// stream order: `slots` slots of n streams in all (one stream: total, count, its pairs, stamps and labels; a sharing bank: its counts
// are 0 -- its state is the total)
static int64_t knn_state_bytes(const htm_knn *knn, int64_t n, int64_t slots) { return 8 * (1 + n) + slots * ((int64_t)knn->d.max_pairs * 8 + 12); }

static int64_t knn_slots(const std::vector<int32_t> &counts) {
    int64_t all = 0;
    for (int32_t c : counts) all += c;
    return all;
}

extern "C" int htm_knn_info(const htm_knn *knn, htm_knn_info_t *out) {
    if (!knn || !out || out->struct_bytes != sizeof(htm_knn_info_t)) return HTM_ERR_ARGUMENT;
    const KnnDev &d = knn->d;
    *out = htm_knn_info_t{(uint32_t)sizeof(htm_knn_info_t), d.labels, d.k, d.min_overlap, d.capacity, d.n_cols * d.K, d.K, d.max_pairs, knn->count, d.in_lds,
                          d.queries, d.shift, knn->total, knn_state_bytes(knn, 1, knn->count), knn->device_bytes};
    return HTM_OK;
}

extern "C" int htm_knns_info(const htm_knn *knn, htm_knns_info_t *out, int32_t *counts) {
    if (!knn || !out || out->struct_bytes != sizeof(htm_knns_info_t) || !knn->is_bank) return HTM_ERR_ARGUMENT;
    const KnnDev &d = knn->d;
    const int64_t scratch = knn->source ? gknn_scratch_bytes(1, knn->chunk, d.capacity, d.words) : gknn_scratch_bytes(knn->n, knn->chunk, d.capacity, d.words);
    *out = htm_knns_info_t{(uint32_t)sizeof(htm_knns_info_t), d.labels, d.k, d.min_overlap, d.capacity, d.n_cols * d.K, d.K, d.max_pairs, knn->n,
                           knn->source ? 1 : 0, knn->chunk, d.in_lds, d.queries, d.shift, knn->source ? knn->source->count : knn->count, 0, knn->total,
                           knn_state_bytes(knn, knn->n, knn_slots(knn->counts)), knn->device_bytes, scratch};
    if (counts)
        for (size_t m = 0; m < (size_t)knn->n; ++m) counts[m] = knn->counts[m];
    return HTM_OK;
}

// the state copied to the host blob (load == 0) or from it, behind everything enqueued on h's stream
static int knn_state(const char *what, bool bank, bool load, htm_knn *knn, htm_handle *h, void *host_state, int64_t bytes) {
    if (int rc = knn_check(what, knn, h, bank)) return rc;
    const std::string w = std::string(what) + ": ";
    const size_t n = (size_t)knn->n;
    const int64_t head_bytes = 8 * (1 + (int64_t)n);
    if (!host_state || bytes < head_bytes)
        return cls_refuse(h, w + "need host_state of " + (bank ? "htm_knns_info" : "htm_knn_info") + "'s state_bytes", HTM_ERR_ARGUMENT);
    const KnnDev &d = knn->d;
    std::vector<int64_t> head(1 + n);
    head[0] = knn->total;
    for (size_t m = 0; m < n; ++m) head[1 + m] = knn->counts[m];
    if (load) memcpy(head.data(), host_state, (size_t)head_bytes);
    std::vector<int32_t> counts(n);
    bool ok = head[0] >= 0;
    for (size_t m = 0; m < n; ++m) {
        ok = ok && head[1 + m] >= 0 && head[1 + m] <= (knn->source ? 0 : d.capacity);
        counts[m] = ok ? (int32_t)head[1 + m] : 0;
    }
    const size_t all = (size_t)knn_slots(counts);
    if (!ok || bytes != knn_state_bytes(knn, (int64_t)n, (int64_t)all))
        return cls_refuse(h, w + (bank ? "need host_state of 8 (1 + n) + the counts x (8 max_pairs + 12) bytes with 0 <= count <= capacity (0 on a shared store), total >= 0"
                                       : "need host_state of 16 + count x (8 max_pairs + 12) bytes with 0 <= count <= capacity, total >= 0"), HTM_ERR_ARGUMENT);
    const size_t row = (size_t)d.max_pairs * 8;
    char *pairs = (char *)host_state + head_bytes, *stamps = pairs + all * row, *labels = stamps + all * 8;
    if (load) {
        size_t at = 0;
        for (size_t m = 0; m < n; ++m) {
            int64_t last = -1;
            for (size_t i = 0; i < (size_t)counts[m]; ++i, ++at) {
                int64_t stamp;
                int32_t label;
                memcpy(&stamp, stamps + at * 8, 8);
                memcpy(&label, labels + at * 4, 4);
                const auto slot = [&] { return (bank ? "stream " + std::to_string(m) + ", " : "") + "slot " + std::to_string(i); };
                if (stamp <= last || stamp >= head[0]) return cls_refuse(h, w + "the stamps must ascend and lie below total (" + slot() + ")", HTM_ERR_ARGUMENT);
                if (label < 0 || label >= d.labels) return cls_refuse(h, w + "a label outside [0, labels) in " + slot(), HTM_ERR_ARGUMENT);
                last = stamp;
            }
        }
    }
    HIPCHK(h, hipSetDevice(knn->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const hipMemcpyKind kind = load ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (!load) memcpy(host_state, head.data(), (size_t)head_bytes);
    size_t at = 0;
    for (size_t m = 0; m < n; ++m) {
        const size_t c = (size_t)counts[m], cap = (size_t)d.capacity;
        if (c) {
            void *dev[3] = {d.store + m * cap * d.max_pairs, d.stamp + m * cap, d.label + m * cap};
            void *host[3] = {pairs + at * row, stamps + at * 8, labels + at * 4};
            const size_t size[3] = {c * row, c * 8, c * 4};
            for (int a = 0; a < 3; ++a) HIPCHK(h, hipMemcpy(load ? dev[a] : host[a], load ? host[a] : dev[a], size[a], kind));
        }
        at += c;
    }
    if (load) {
        knn->total = head[0];
        knn->counts = counts;
        knn->count = n ? *std::max_element(counts.begin(), counts.end()) : 0;
    }
    return HTM_OK;
}

extern "C" int htm_knn_export(htm_knn *knn, htm_handle *h, void *host_state, int64_t bytes) { return knn_state("htm_knn_export", false, false, knn, h, host_state, bytes); }
extern "C" int htm_knn_import(htm_knn *knn, htm_handle *h, const void *host_state, int64_t bytes) {
    return knn_state("htm_knn_import", false, true, knn, h, (void *)host_state, bytes);
}
extern "C" int htm_knns_export(htm_knn *knn, htm_handle *h, void *host_state, int64_t bytes) { return knn_state("htm_knns_export", true, false, knn, h, host_state, bytes); }
extern "C" int htm_knns_import(htm_knn *knn, htm_handle *h, const void *host_state, int64_t bytes) {
    return knn_state("htm_knns_import", true, true, knn, h, (void *)host_state, bytes);
}

// ------------------------------------------------------------------------------------------
// Live ticks (htm_live.h): the group's staging and result blocks, allocated by the first live call
static int live_alloc(htm_group *g, size_t cls_need = 0) {
    htm_group::Live &lv = g->live;
    if (lv.vote_tab && cls_need <= lv.cls_cap) return 0;
    const Dev &d = g->m[0]->d;
    const size_t n = (size_t)g->n;
    if (!lv.vote_tab) {
        lv.off_flags = n * (size_t)d.W * 4;             // (W is a multiple of 4 words: the flags and the values stay 8-byte aligned)
        lv.off_values = (lv.off_flags + n * 4 + 7) & ~(size_t)7;
        // (... a classified tick's targets, and a tick with a KNN bank's labels, counts and slots: four words per member)
        lv.stage_bytes = lv.off_values + n * HTM_SCALAR_MAX_FIELDS * sizeof(double) + n * sizeof(int32_t) + n * 4 * sizeof(int32_t);
        if (!lv.h_stage && hipHostMalloc((void **)&lv.h_stage, lv.stage_bytes, hipHostMallocDefault) != hipSuccess) { lv.h_stage = nullptr; g->err = "live tick: hipHostMalloc failed"; return HTM_ERR_HIP; }
        memset(lv.h_stage, 0, lv.stage_bytes);          // (the words of a staged row beyond ceil(input_dim / 32) stay zero)
        if (!lv.d_stage && galloc(g, &lv.d_stage, lv.stage_bytes)) return HTM_ERR_HIP;
        if (!lv.d_recs && galloc(g, &lv.d_recs, n)) return HTM_ERR_HIP;
        if (!lv.bank_tab && galloc(g, (uint32_t ***)&lv.bank_tab, n)) return HTM_ERR_HIP;
        if (!lv.rec_args && galloc(g, &lv.rec_args, n)) return HTM_ERR_HIP;
        std::vector<const uint32_t *> banks(n);
        std::vector<GrpRecArgs> recs(n);
        for (size_t i = 0; i < n; ++i) {
            banks[i] = (const uint32_t *)lv.d_stage + i * (size_t)d.W;
            recs[i] = GrpRecArgs{lv.d_recs + i, nullptr, nullptr};
        }
        GHIPCHK(g, hipMemset(lv.d_stage, 0, lv.stage_bytes));
        GHIPCHK(g, hipMemcpy((void *)lv.bank_tab, banks.data(), n * sizeof(uint32_t *), hipMemcpyHostToDevice));
        GHIPCHK(g, hipMemcpy(lv.rec_args, recs.data(), n * sizeof(GrpRecArgs), hipMemcpyHostToDevice));
    } else {
        // a classified tick that needs more room in front of the likelihoods: the result block anew (nothing enqueued reads the old one
        // behind the wait; the vote table keeps its address, which is all the tick's graphs hold)
        GHIPCHK(g, hipStreamSynchronize(g->stream));
        hipHostFree(lv.h_out);
        g->allocs.erase(std::remove(g->allocs.begin(), g->allocs.end(), (void *)lv.d_out), g->allocs.end());
        hipFree(lv.d_out);
        lv.h_out = lv.d_out = nullptr;
    }
    lv.cls_cap = (cls_need + 7) & ~(size_t)7;
    lv.off_lik = lv.cls_cap;
    lv.off_rows = lv.off_lik + n * sizeof(double);
    lv.off_pairs = lv.off_rows + n * sizeof(htm_live_row);
    lv.off_votes = lv.off_pairs + n * HTM_SCALAR_MAX_FIELDS * 2 * sizeof(int32_t);
    lv.out_bytes = lv.off_votes + n * (size_t)d.I * sizeof(int32_t);
    if (!lv.h_out && hipHostMalloc((void **)&lv.h_out, lv.out_bytes, hipHostMallocDefault) != hipSuccess) { lv.h_out = nullptr; g->err = "live tick: hipHostMalloc failed"; return HTM_ERR_HIP; }
    memset(lv.h_out, 0, lv.out_bytes);
    if (!lv.d_out && galloc(g, &lv.d_out, lv.out_bytes)) return HTM_ERR_HIP;
    int32_t **vote_tab = lv.vote_tab;
    if (!vote_tab && galloc(g, &vote_tab, n)) return HTM_ERR_HIP;
    std::vector<int32_t *> votes(n);
    for (size_t i = 0; i < n; ++i) votes[i] = (int32_t *)(lv.d_out + lv.off_votes) + i * (size_t)d.I;
    GHIPCHK(g, hipMemset(lv.d_out, 0, lv.out_bytes));
    GHIPCHK(g, hipMemcpy(vote_tab, votes.data(), n * sizeof(int32_t *), hipMemcpyHostToDevice));
    lv.vote_tab = vote_tab;
    return 0;
}

// the rows a classified tick captures its members' patterns into, and the table of their descriptors, allocated by the first such tick
static int live_alloc_capture(htm_group *g) {
    htm_group::Live &lv = g->live;
    if (lv.d_caps) return 0;
    const Dev &d = g->m[0]->d;
    const size_t n = (size_t)g->n, per = (size_t)d.k * d.WPC;
    if (!lv.cap_rows && galloc(g, &lv.cap_rows, n * per)) return HTM_ERR_HIP;
    ClsCapDev *caps = nullptr;
    if (galloc(g, &caps, n)) return HTM_ERR_HIP;
    std::vector<ClsCapDev> rows(n);
    for (size_t i = 0; i < n; ++i) rows[i].rows = lv.cap_rows + i * per;
    GHIPCHK(g, hipMemcpy(caps, rows.data(), n * sizeof(ClsCapDev), hipMemcpyHostToDevice));
    lv.d_caps = caps;
    return 0;
}

// One tick of every member.  Per member the host only checks arguments, fills its part of the pinned staging block and, after the
// one wait, copies its results out and notes its segment count (what hand_back_segments leaves for the next call's scan).
static int live_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                     const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                     htm_likelihood *lk, double *likelihood, htm_classifier *clf = nullptr, const int32_t *targets = nullptr, int32_t cls_learn = 0,
                     int32_t *best = nullptr, int32_t *dist = nullptr, htm_knn *knn = nullptr, const int32_t *knn_labels = nullptr, int32_t knn_learn = 0,
                     int32_t *knn_best = nullptr, int32_t *knn_votes = nullptr) {
    if (!g) return HTM_ERR_ARGUMENT;
    if (!rows) { g->err = "htm_live_tick: null rows"; return HTM_ERR_ARGUMENT; }
    // a classified tick (htm_classifiers_tick): every refusal before anything is enqueued
    if ((clf != nullptr) != (best != nullptr) || (clf != nullptr) != (targets != nullptr) || (dist && !clf)) {
        g->err = "htm_classifiers_tick: clf, targets and best go together (dist only with them)";
        return HTM_ERR_ARGUMENT;
    }
    if (clf) {
        const Dev &d0 = g->m[0]->d;
        const ClsDev &c = clf->d;
        if (clf->n != g->n || clf->device != g->device) {
            g->err = "htm_classifiers_tick: the classifier has " + std::to_string(clf->n) + " streams on device " + std::to_string(clf->device) + ", the group " +
                     std::to_string(g->n) + " members on device " + std::to_string(g->device);
            return HTM_ERR_ARGUMENT;
        }
        if (c.n_cols != d0.C || c.K != d0.K || c.max_pairs < d0.k * d0.WPC) {
            g->err = "htm_classifiers_tick: the classifier was made for " + std::to_string(c.n_cols) + " columns of " + std::to_string(c.K) + " cells and patterns of " +
                     std::to_string(c.max_pairs) + " pairs, the members have " + std::to_string(d0.C) + " x " + std::to_string(d0.K) + " and " +
                     std::to_string(d0.k * d0.WPC) + " pairs a step";
            return HTM_ERR_ARGUMENT;
        }
        if (cls_learn && clf->shares) { g->err = "htm_classifiers_tick: the streams read another object's weights: learn must be 0"; return HTM_ERR_STATE; }
        for (int i = 0; i < g->n; ++i)
            if (int rc = pin_refuse(g->m[i], "htm_classifiers_tick")) { g->err = "member " + std::to_string(i) + ": " + g->m[i]->err; return rc; }
    }
    // a tick with a bank of KNN classifiers (htm_knns_tick): likewise.  The host knows every label, so it knows every stream's slot
    std::vector<int32_t> knn_after;
    int32_t knn_largest = 0;
    bool knn_stores = false;
    if ((knn != nullptr) != (knn_best != nullptr) || ((knn_labels || knn_learn || knn_votes) && !knn)) {
        g->err = "htm_knns_tick: knn and knn_best go together (labels, knn_learn and knn_votes only with them)";
        return HTM_ERR_ARGUMENT;
    }
    if (knn) {
        const Dev &d0 = g->m[0]->d;
        const KnnDev &c = knn->d;
        if (!knn->is_bank) { g->err = "htm_knns_tick: the object is a one-stream KNN classifier: a tick takes a bank (htm_knns_create)"; return HTM_ERR_ARGUMENT; }
        if (knn->n != g->n || knn->device != g->device) {
            g->err = "htm_knns_tick: the bank has " + std::to_string(knn->n) + " streams on device " + std::to_string(knn->device) + ", the group " +
                     std::to_string(g->n) + " members on device " + std::to_string(g->device);
            return HTM_ERR_ARGUMENT;
        }
        if (c.n_cols != d0.C || c.K != d0.K || c.max_pairs < d0.k * d0.WPC) {
            g->err = "htm_knns_tick: the bank was made for " + std::to_string(c.n_cols) + " columns of " + std::to_string(c.K) + " cells and patterns of " +
                     std::to_string(c.max_pairs) + " pairs, the members have " + std::to_string(d0.C) + " x " + std::to_string(d0.K) + " and " +
                     std::to_string(d0.k * d0.WPC) + " pairs a step";
            return HTM_ERR_ARGUMENT;
        }
        if (knn_learn && knn->source) { g->err = "htm_knns_tick: the streams read another object's store: learn must be 0"; return HTM_ERR_STATE; }
        if (knn_learn && !knn_labels) { g->err = "htm_knns_tick: a learning tick needs the members' labels"; return HTM_ERR_ARGUMENT; }
        knn_after = knn->counts;
        for (int i = 0; i < g->n; ++i) {
            const bool labelled = knn_learn && knn_labels[i] >= 0 && knn_labels[i] < c.labels;
            if (labelled && knn->counts[(size_t)i] + 1 > c.capacity) {
                g->err = "htm_knns_tick: stream " + std::to_string(i) + ": the tick would store 1 pattern in a store of " + std::to_string(knn->counts[(size_t)i]) +
                         " of capacity = " + std::to_string(c.capacity) + " slots";
                return HTM_ERR_CAPACITY;
            }
            knn_after[(size_t)i] += labelled;
            knn_stores |= labelled;
            knn_largest = std::max(knn_largest, knn_after[(size_t)i]);
        }
        for (int i = 0; i < g->n; ++i)
            if (int rc = pin_refuse(g->m[i], "htm_knns_tick")) { g->err = "member " + std::to_string(i) + ": " + g->m[i]->err; return rc; }
    }
    if ((lk != nullptr) != (likelihood != nullptr)) { g->err = "htm_likelihood_tick: lk and likelihood go together"; return HTM_ERR_ARGUMENT; }
    if (lk && (lk->n != g->n || lk->device != g->device)) {
        g->err = "htm_likelihood_tick: the likelihood object has " + std::to_string(lk->n) + " streams on device " + std::to_string(lk->device) +
                 ", the group " + std::to_string(g->n) + " members on device " + std::to_string(g->device);
        return HTM_ERR_ARGUMENT;
    }
    if ((values != nullptr) == (packed_inputs != nullptr)) { g->err = "htm_live_tick: give either values (with a field table) or packed_inputs"; return HTM_ERR_ARGUMENT; }
    htm_handle *h0 = g->m[0];
    ScalarTab ftab;
    memset(&ftab, 0, sizeof(ftab));
    if (values) {
        if (int rc = scalar_table(h0, "htm_live_tick", fields, n_fields, decoded != nullptr, &ftab)) { g->err = h0->err; return rc; }
    } else if (fields || n_fields || decoded) {
        g->err = "htm_live_tick: a field table and decoded pairs go with values, not with packed_inputs";
        return HTM_ERR_ARGUMENT;
    }
    if (learning && g->has_view) { g->err = "htm_live_tick: a group with inference views steps with learning = 0 only"; return HTM_ERR_STATE; }
    int rc = group_check(g, nullptr, nullptr);
    if (rc) return rc;
    GHIPCHK(g, hipSetDevice(g->device));
    rc = group_join(g);
    if (rc) return rc;
    // (the classification's bytes in the result block: best, then dist)
    const size_t best_bytes = clf ? (size_t)g->n * clf->d.H * 2 * sizeof(int32_t) : 0, dist_bytes = dist ? (size_t)g->n * clf->d.H * clf->d.B * sizeof(int32_t) : 0;
    // (... and behind them a KNN bank's rows [B][5] and votes [B][labels])
    const size_t knn_best_bytes = knn ? (size_t)g->n * 5 * sizeof(int32_t) : 0, knn_votes_bytes = knn_votes ? (size_t)g->n * knn->d.labels * sizeof(int32_t) : 0;
    const size_t cls_bytes = (best_bytes + dist_bytes + knn_best_bytes + knn_votes_bytes + 7) & ~(size_t)7;
    rc = live_alloc(g, cls_bytes);
    if (rc) return rc;
    if (clf || knn) {
        rc = live_alloc_capture(g);
        if (rc) return rc;
    }
    if (clf) {
        if (cls_prepare(clf, h0, cls_learn, 1)) { g->err = h0->err; return HTM_ERR_HIP; }
    }
    htm_group::Live &lv = g->live;
    const Dev &d = h0->d;
    const hipStream_t s = g->stream;
    const int B = g->n, p = (int)(h0->step_host & 1);
    const int n_dec = decoded ? (int)n_fields : 0;
    learning = learning ? 1 : 0;
    // the one copy in: the rows and the flags (a contiguous part of the block), or the flags and the values
    int32_t *flags = (int32_t *)(lv.h_stage + lv.off_flags);
    bool resetting = false;
    for (int i = 0; i < B; ++i) {
        flags[i] = resets && resets[i] ? LIVE_RESET | (p ? LIVE_PARITY : 0) : 0;
        resetting |= flags[i] != 0;
    }
    size_t c0, c1;
    if (values) {
        memcpy(lv.h_stage + lv.off_values, values, (size_t)B * n_fields * sizeof(double));
        c0 = lv.off_flags;
        c1 = lv.off_values + (size_t)B * n_fields * sizeof(double);
    } else {
        const size_t words = (size_t)(d.I + 31) / 32;
        for (int i = 0; i < B; ++i) memcpy(lv.h_stage + (size_t)i * d.W * 4, packed_inputs + (size_t)i * words, words * 4);
        c0 = 0;
        c1 = lv.off_flags + (size_t)B * 4;
    }
    // a classified tick's targets ride behind them in the same copy (a tick of packed rows: where the values would lie)
    const size_t off_targets = values ? c1 : lv.off_values;
    if (clf) {
        memcpy(lv.h_stage + off_targets, targets, (size_t)B * sizeof(int32_t));
        c1 = off_targets + (size_t)B * sizeof(int32_t);
    }
    // ... and behind those a KNN bank's words: every member's label [B], its stream's counts before and behind the tick [B][2] and the
    // slot its pattern goes into [B] (-1: it stores nothing)
    const size_t off_knn = c1;
    if (knn && !knn->source) {
        int32_t *w = (int32_t *)(lv.h_stage + off_knn);
        for (int i = 0; i < B; ++i) {
            const bool stores = knn_after[(size_t)i] != knn->counts[(size_t)i];
            w[i] = stores ? knn_labels[i] : -1;
            w[B + 2 * i] = knn->counts[(size_t)i];
            w[B + 2 * i + 1] = knn_after[(size_t)i];
            w[3 * B + i] = stores ? knn->counts[(size_t)i] : -1;
        }
        c1 = off_knn + (size_t)B * 4 * sizeof(int32_t);
    }
    GHIPCHK(g, hipMemcpyAsync(lv.d_stage + c0, lv.h_stage + c0, c1 - c0, hipMemcpyHostToDevice, s));
    // resets first: the record's begin launch then counts the cleared prediction words (predicted_columns_before = 0)
    if (resetting) LAUNCH_ON(h0, s, 0, "live:reset", klive_reset, dim3(reset_blocks(d), B), 256, g->d_tab, (const int32_t *)(lv.d_stage + lv.off_flags));
    LAUNCH_ON(h0, s, 0, "group:record", kgrp_rec_clear, B, 64, g->d_recs);
    LAUNCH_ON(h0, s, 0, "group:record", kgrp_rec_begin, dim3(rec_blocks(d), B), 256, g->d_tab, p ^ 1, g->d_recs, (const GrpRecArgs *)lv.rec_args, 1);
    const FieldPath path = values ? field_path(ftab, n_fields) : FIELDS_LINEAR;       // (the table's kernels: htm_scalar.h, htm_fields.h or htm_coord.h)
    if (values)
        LAUNCH_ON(h0, s, 0, "live:encode", encode_kernel(path), B, encode_threads(path, d.W), d, ftab, (int)n_fields, (const double *)(lv.d_stage + lv.off_values),
                  (uint32_t *)lv.d_stage, 0);
    const bool decoding = decoded || votes;
    if (decoding) LAUNCH_ON(h0, s, 0, "group:predicted_input", kgrp_pin_begin, dim3(pin_begin_blocks(1, d.I), B), 256, g->d_tab, p ^ 1, g->d_pins, lv.vote_tab, 1);
    const RunModes modes{true, false, decoding, false, clf != nullptr || knn != nullptr};     // (a classified tick captures its step's patterns, once)
    GroupForm f = group_form(g);
    f.shared = g->shared && !learning;
    if (run_schedule(h0, 1, use_graph).graph) {
        const GroupGraphKey key{p, modes, learning, f.fuse, f.large, f.shared, f.spec, 1, lv.bank_tab, 1};
        const hipGraphExec_t exec = cached_graph(g->graphs, key, s, g->err, [&] {
            group_enqueue_step(g, modes, lv.bank_tab, 1, learning, p, f, lv.d_caps);
            return 0;
        });
        if (!exec) return HTM_ERR_HIP;
        GHIPCHK(g, hipGraphLaunch(exec, s));
    } else {
        group_enqueue_step(g, modes, lv.bank_tab, 1, learning, p, f, lv.d_caps);
    }
    LAUNCH_ON(h0, s, 0, "live:finish", finish_kernel(path), dim3(std::max(n_dec, 1), B), SCALAR_THREADS, g->d_tab, p, ftab, n_dec,
              (const int32_t *)(lv.d_out + lv.off_votes), (const htm_step_record *)lv.d_recs, (htm_live_row *)(lv.d_out + lv.off_rows),
              (int32_t *)(lv.d_out + lv.off_pairs));
    // a scored tick: every member's stream of the likelihood object takes the step's record, behind the finish launch
    if (lk) LAUNCH_ON(h0, s, 0, "live:likelihood", klik_tick, dim3(1, B), HTM_LIKELIHOOD_THREADS, lk->d, (const htm_step_record *)lv.d_recs, (double *)(lv.d_out + lv.off_lik));
    // a classified tick: every member's stream of the bank takes the step's captured pattern -- sum + apply when it learns, else the
    // frozen launch over one step; a member's reset flag (bit 0 of its word) also empties its stream's history
    const size_t cls_begin = lv.off_lik - cls_bytes;
    if (clf) {
        GClsStep gs;
        memset(&gs, 0, sizeof(gs));
        gs.pairs = lv.cap_rows;
        gs.pairs_stride = (int64_t)d.k * d.WPC;
        gs.targets = (const int32_t *)(lv.d_stage + off_targets);
        gs.targets_stride = 1;
        gs.reset_bits = (const uint32_t *)(lv.d_stage + lv.off_flags);
        gs.resets_stride = 1;
        gs.pairs_per_step = d.k * d.WPC;
        gs.n_targets = 1;
        gs.first_step = 0;
        gs.n_steps = 1;
        gs.best = (int32_t *)(lv.d_out + cls_begin);
        gs.dist = dist ? (int32_t *)(lv.d_out + cls_begin + best_bytes) : nullptr;
        if (cls_enqueue(clf, h0, s, gs, cls_learn)) { g->err = h0->err; return HTM_ERR_HIP; }
    }
    // a tick with a KNN bank: every member's stream takes the step's captured pattern -- append (when any stream stores: the slots came
    // in the staging copy, there is no place launch), distance, select; the frozen streams of a shared store are one flat batch of B
    // queries.  A member's reset flag does not touch its store: the store is not sequence state.
    const size_t knn_begin = cls_begin + best_bytes + dist_bytes;
    if (knn) {
        int32_t *out_best = (int32_t *)(lv.d_out + knn_begin), *out_votes = knn_votes ? (int32_t *)(lv.d_out + knn_begin + knn_best_bytes) : nullptr;
        const int32_t per = d.k * d.WPC;
        if (knn->source) {
            if (knns_enqueue_shared(knn, h0, s, lv.cap_rows, per, B, out_best, out_votes)) { g->err = h0->err; return HTM_ERR_HIP; }
        } else {
            const int32_t *w = (const int32_t *)(lv.d_stage + off_knn);
            GKnnStep gs{};
            gs.s = KnnStep{lv.cap_rows, per, w, 1, 0, 1, out_best, out_votes, knn->total, 0, 0};
            gs.pairs = nullptr;
            gs.pairs_stride = per;
            gs.counts = w + B;
            gs.pos = (int32_t *)(lv.d_stage + off_knn) + 3 * B;
            if (knns_enqueue(knn, h0, s, gs, knn_largest, knn_stores, false)) { g->err = h0->err; return HTM_ERR_HIP; }
            knn->counts = knn_after;
            knn->count = knn_largest;
        }
        knn->total += 1;
    }
    for (htm_handle *h : g->m) {
        h->step_host += 1;
        h->window_known = true;
        if (learning) weights_touched(h);
    }
    rc = launch_status(g->err);
    if (rc) return rc;
    // the one copy out and the one wait
    const size_t pair_bytes = (size_t)B * n_dec * 2 * sizeof(int32_t), vote_bytes = (size_t)B * d.I * sizeof(int32_t);
    const size_t out_end = votes ? lv.off_votes + vote_bytes : lv.off_pairs + pair_bytes, out_begin = clf || knn ? cls_begin : lk ? lv.off_lik : lv.off_rows;
    GHIPCHK(g, hipMemcpyAsync(lv.h_out + out_begin, lv.d_out + out_begin, out_end - out_begin, hipMemcpyDeviceToHost, s));
    GHIPCHK(g, hipStreamSynchronize(s));
    memcpy(rows, lv.h_out + lv.off_rows, (size_t)B * sizeof(htm_live_row));
    if (lk) memcpy(likelihood, lv.h_out + lv.off_lik, (size_t)B * sizeof(double));
    if (clf) memcpy(best, lv.h_out + cls_begin, best_bytes);
    if (dist) memcpy(dist, lv.h_out + cls_begin + best_bytes, dist_bytes);
    if (knn) memcpy(knn_best, lv.h_out + knn_begin, knn_best_bytes);
    if (knn_votes) memcpy(knn_votes, lv.h_out + knn_begin + knn_best_bytes, knn_votes_bytes);
    if (decoded) memcpy(decoded, lv.h_out + lv.off_pairs, pair_bytes);
    if (votes) memcpy(votes, lv.h_out + lv.off_votes, vote_bytes);
    for (int i = 0; i < B; ++i) {                   // (the segment hint each member's next call -- group or solo -- starts from)
        htm_handle *h = g->m[i];
        h->seg_hint = std::max(h->seg_hint, (int)rows[i].record.segments);
        if (h->seg_pinned) *h->seg_pinned = rows[i].record.segments;
    }
    return HTM_OK;
}

extern "C" int htm_live_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                             const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes) {
    return live_tick(g, values, fields, n_fields, packed_inputs, resets, learning, use_graph, rows, decoded, votes, nullptr, nullptr);
}

extern "C" int htm_likelihood_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                                   const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                                   htm_likelihood *lk, double *likelihood) {
    return live_tick(g, values, fields, n_fields, packed_inputs, resets, learning, use_graph, rows, decoded, votes, lk, likelihood);
}

// htm_likelihood_tick with a bank of classifiers riding on it (lk and likelihood may be NULL: an unscored, classified tick)
extern "C" int htm_classifiers_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                                    const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                                    htm_likelihood *lk, double *likelihood, htm_classifier *clf, const int32_t *targets, int32_t learn, int32_t *best,
                                    int32_t *dist) {
    return live_tick(g, values, fields, n_fields, packed_inputs, resets, learning, use_graph, rows, decoded, votes, lk, likelihood, clf, targets, learn ? 1 : 0,
                     best, dist);
}

// htm_classifiers_tick with a bank of KNN classifiers riding on it (lk, likelihood and the classifier's arguments may be NULL)
extern "C" int htm_knns_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                             const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                             htm_likelihood *lk, double *likelihood, htm_classifier *clf, const int32_t *targets, int32_t learn, int32_t *best, int32_t *dist,
                             htm_knn *knn, const int32_t *labels, int32_t knn_learn, int32_t *knn_best, int32_t *knn_votes) {
    if (g && !knn) { g->err = "htm_knns_tick: null knn"; return HTM_ERR_ARGUMENT; }
    return live_tick(g, values, fields, n_fields, packed_inputs, resets, learning, use_graph, rows, decoded, votes, lk, likelihood, clf, targets, learn ? 1 : 0,
                     best, dist, knn, labels, knn_learn ? 1 : 0, knn_best, knn_votes);
}

// htm_reset of the flagged members in one launch.  The flags are the call's own (pageable) words: the copy has read them when
// it returns, as the staging copy of htm_group_step.
extern "C" int htm_live_reset(htm_group *g, const uint8_t *members) {
    if (!g) return HTM_ERR_ARGUMENT;
    std::vector<int32_t> flags((size_t)g->n, 0);
    bool any = false;
    for (int i = 0; i < g->n; ++i) {
        if (members && !members[i]) continue;
        const htm_handle *h = g->m[i];
        const std::string who = "htm_live_reset: member " + std::to_string(i);
        if (sp_is_ahead(h)) { g->err = who + ": the Spatial Pooler is ahead (htm_run ended with HTM_RUN_CONTINUE)"; return HTM_ERR_STATE; }
        if (h->shard_open) { g->err = who + " has a step open"; return HTM_ERR_STATE; }
        flags[i] = LIVE_RESET | ((h->step_host & 1) ? LIVE_PARITY : 0);
        any = true;
    }
    if (!any) return HTM_OK;
    GHIPCHK(g, hipSetDevice(g->device));
    for (int i = 0; i < g->n; ++i) {                // (the flagged members' own work first, as htm_reset: tails, open phases)
        if (!flags[i]) continue;
        htm_handle *h = g->m[i];
        flush_tail(h);
        if (int rc = view_enter(h, 0)) { g->err = h->err; return rc; }
        if (close_open_phases(h)) { g->err = h->err; return HTM_ERR_HIP; }
        if (h->stream != g->stream) GHIPCHK(g, hipStreamSynchronize(h->stream));
    }
    if (int rc = live_alloc(g)) return rc;
    htm_group::Live &lv = g->live;
    htm_handle *h0 = g->m[0];
    const hipStream_t s = g->stream;
    GHIPCHK(g, hipMemcpyAsync(lv.d_stage + lv.off_flags, flags.data(), flags.size() * 4, hipMemcpyHostToDevice, s));
    LAUNCH_ON(h0, s, 0, "live:reset", klive_reset, dim3(reset_blocks(h0->d), g->n), 256, g->d_tab, (const int32_t *)(lv.d_stage + lv.off_flags));
    const int rc = launch_status(g->err);
    if (rc) return rc;
    if (g->mixed) GHIPCHK(g, hipStreamSynchronize(s));
    return HTM_OK;
}
