// Per-step record of a recorded htm_run (htm_run_recorded, include/bithtm_hip.h): one launch behind each recorded step's
// last launch, and one before the call's first step.
//
// Where each count is taken:
//   active_columns, active_column   the step's winner list active_cols[p] (k entries, ascending)
//   bursting_columns                the activation role's per-column flags d.bursting[0..k)
//   predicted_columns, prediction   pred[p] once the step's scan has set its last bit (this launch follows the scan)
//   predicted_columns_before        the count the previous recorded step left in RecDev::prev_pred, or, for the first step of
//                                   a call, the count k_rec_begin took of the last completed step's pred words
//   active_cells, winner_cells, segments, new_segments   the counters the step's roles leave in the counter block
//                                   (n_active_cells, n_win[p], S, n_un ? n_recycled + n_new : 0 -- what htm_get_info reports)
// The launch runs after step t's last launch and before step t+1's first one, so every buffer it reads still holds step t:
// the look-ahead of the pipelined schedules writes the other parity's winner list and never touches pred[p] or the
// counters of step t.  Nothing is recorded for a step outside [base, base + n).

// blocks of both record launches (enough that every winner-list entry has a thread: see rec_blocks), passes of a wave's
// prediction words whose loads are issued together
#define REC_BLOCKS_MIN 32
#define REC_UNROLL 8

// device-side descriptor of the current recorded call (one per handle; graphs of recorded steps hold its address, the
// call's k_rec_begin fills it)
struct RecDev {
    htm_step_record *rec;      // [n] or null
    int32_t *cols;             // [n * k] or null
    uint32_t *colpred;         // [n * ceil(C / 32)] or null
    uint32_t base;             // step index of record 0
    int32_t n;                 // records of this call
    int32_t prev_pred;         // predicted columns of the last step (recorded, or counted by k_rec_begin)
    uint32_t pad;
    u64 acc;                   // per-step reduction across the blocks of k_rec_step, zero between launches: predicted columns
                               // (bits 0-23) | bursting columns << 24 | blocks arrived << 48 -- one atomic per block carries all three
};

// columns [c0, c0 + 64) of the wave: bit = any predicted cell of the column (pred words of parity q)
__device__ __forceinline__ u64 rec_column_bits(const Dev &d, int q, int c) {
    uint32_t any = 0;
    if (c < d.C)
        for (int h = 0; h < d.WPC; ++h) any |= d.pred[q][c * d.WPC + h];
    return __ballot(any != 0);
}

// Before the call's first launch (the descriptor was zeroed just before): the pointers, and the count of the columns the
// last completed step (parity q) predicts -- a fresh handle's zeroed words, an imported state's, those of htm_step /
// htm_tm_scan / an unrecorded run alike.  REC_BLOCKS blocks, one atomic each into prev_pred.
// (the body of both record launches is a role of its own: the model-group launches of htm_group.h call it for their members)
__device__ __forceinline__ void role_rec_begin(const Dev &d, int q, RecDev *r, htm_step_record *rec, int32_t *cols, uint32_t *colpred,
                                               uint32_t base, int32_t n) {
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t cnt = 0;
    for (int c0 = (int)(blockIdx.x * 256 + (threadIdx.x & ~63)); c0 < d.C; c0 += (int)gridDim.x * 256)
        cnt += (uint32_t)__popcll(rec_column_bits(d, q, c0 + lane_id()));
    if (lane_id() == 0 && cnt) atomicAdd(&s_n, cnt);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd((uint32_t *)&r->prev_pred, s_n);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r->rec = rec;
        r->cols = cols;
        r->colpred = colpred;
        r->base = base;
        r->n = n;
    }
}

__global__ __launch_bounds__(256) void k_rec_begin(Dev d, int q, RecDev *r, htm_step_record *rec, int32_t *cols, uint32_t *colpred,
                                                   uint32_t base, int32_t n) {
    role_rec_begin(d, q, r, rec, cols, colpred, base, n);
}

// Behind step p's last launch: REC_BLOCKS blocks of 256 threads, a thread per column per pass (and, below k, per winner-list
// entry).  Every load a thread makes is issued before the first result is used: the winner-list entry and bursting flag, the
// counters the record copies (thread 0; nothing in this launch writes them), and up to REC_UNROLL passes of prediction
// words -- one memory round trip for the whole pass instead of one per pass.  Per wave: the ballot of predicted columns (two
// words of the packed prediction) and its popcount; per block: ONE 64-bit atomic carrying both counts (predicted columns
// low, bursting columns in the middle, the block's arrival high: RecDev::acc), whose returned value tells the last block to
// arrive the totals; it writes the record and leaves the descriptor clean for the next step.  (DESIGN.md section 9 has the measurements.)
// n_active: entries of the step's winner list (d.k; a stand-alone Temporal Memory run may step with fewer: htm_tm_feed.h -- the
// record then says n_active, and the slots of the active_column row behind them hold -1)
__device__ __forceinline__ void role_rec_step(const Dev &d, int p, RecDev *r, int n_active) {
    __shared__ uint32_t s_pred, s_burst;
    const uint32_t slot = d.ctr->step[p] - r->base;
    if (slot >= (uint32_t)r->n) return;           // (the same answer in every block: nothing is counted, nothing written)
    const Counters *c = d.ctr;
    htm_step_record o;
    if (threadIdx.x == 0) {
        s_pred = 0;
        s_burst = 0;
        o.active_columns = n_active;
        o.predicted_columns_before = r->prev_pred;
        o.active_cells = c->n_active_cells;
        o.winner_cells = c->n_win[p];
        o.segments = c->S;
        o.new_segments = c->n_un ? c->n_recycled + c->n_new : 0;
    }
    const int stride = (int)gridDim.x * 256, i0 = (int)(blockIdx.x * 256 + threadIdx.x);
    const bool has_i = i0 < d.k;                  // (grid >= k / 256 blocks: one entry per thread at most)
    const bool listed = i0 < n_active;            // (n_active <= k)
    const int col = listed ? d.active_cols[p][i0] : -1;
    const bool burst = listed && d.bursting[i0];
    const int words = (d.C + 31) >> 5;
    uint32_t *out = r->colpred ? r->colpred + (size_t)slot * words : nullptr;
    uint32_t n_pred = 0;
    const int wave0 = (int)(blockIdx.x * 256 + (threadIdx.x & ~63));
    for (int base = wave0; base < d.C; base += REC_UNROLL * stride) {
        uint32_t any[REC_UNROLL];
#pragma unroll
        for (int u = 0; u < REC_UNROLL; ++u) {
            const int cc = base + u * stride + lane_id();
            uint32_t a = 0;
            if (cc < d.C) {
                a = d.pred[p][cc * d.WPC];
                if (d.WPC == 2) a |= d.pred[p][cc * 2 + 1];
            }
            any[u] = a;
        }
#pragma unroll
        for (int u = 0; u < REC_UNROLL; ++u) {
            const int c0 = base + u * stride;
            if (c0 >= d.C) break;                 // (uniform across the wave)
            const u64 bits = __ballot(any[u] != 0);
            if (lane_id() == 0) {
                if (out) {
                    out[c0 >> 5] = (uint32_t)bits;
                    if (c0 + 32 < d.C) out[(c0 >> 5) + 1] = (uint32_t)(bits >> 32);
                }
                n_pred += (uint32_t)__popcll(bits);
            }
        }
    }
    __syncthreads();                              // (s_pred / s_burst cleared)
    if (has_i && r->cols) r->cols[(size_t)slot * d.k + i0] = col;
    const uint32_t n_burst = (uint32_t)__popcll(__ballot(burst));
    if (lane_id() == 0 && (n_pred | n_burst)) {
        if (n_pred) atomicAdd(&s_pred, n_pred);
        if (n_burst) atomicAdd(&s_burst, n_burst);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const u64 mine = (u64)s_pred | ((u64)s_burst << 24) | (1ull << 48);
    const u64 acc = atomicAdd(&r->acc, mine) + mine;
    if ((uint32_t)(acc >> 48) != gridDim.x) return;
    o.predicted_columns = (int32_t)(acc & 0xFFFFFFu);
    o.bursting_columns = (int32_t)((acc >> 24) & 0xFFFFFFu);
    if (r->rec) r->rec[slot] = o;
    r->prev_pred = o.predicted_columns;
    r->acc = 0;
}

__global__ __launch_bounds__(256) void k_rec_step(Dev d, int p, RecDev *r) { role_rec_step(d, p, r, d.k); }
