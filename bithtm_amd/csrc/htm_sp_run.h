// Batched stand-alone Spatial Pooler runs (htm_sp_run; include/bithtm_hip.h): the device-side descriptor of
// a recorded call, the launch that fills it, and the launch at the tail of a step.
//
// A step of the run is the front and the back of htm_sp_step (overlap + boost + histogram, select digits where they are
// launched, count + emit: enqueue_sp_front / enqueue_sp_back) and then ONE launch, k_sp_run_tail, in place of k_sp_learn:
//   blocks [0, n_learn)                  DenseProjection.update (projections.py:23-24) on the k winner rows, one row per block:
//                                        role_sp_learn_row, the body of k_sp_learn (n_learn = k when learning, else 0)
//   blocks [n_learn, n_learn + n_rec)    the step's record: thread i < k copies the i-th winner, its overlap and its boosted
//                                        overlap into the call's buffers (n_rec = ceil(k / 256) when recording, else 0)
// The two kinds of block need no order between them: the record blocks read what the select and the overlap left (the winner
// list, overlap[p], boosted[p], the step counter), the learning blocks write permanence and mask rows and read the winner list
// and the bank.  No block waits for another, nothing is an atomic, and the record blocks use no LDS.
// Nothing depends on the step index but through the counter block (step[p]: the emit before this launch wrote step[p ^ 1] only),
// so a captured graph of these launches replays for any step, and -- the buffers and the base step being read from the
// descriptor -- for any recorded call.

// device-side descriptor of the current recorded htm_sp_run call (one per handle; graphs of recorded steps hold its address,
// the call's k_sp_run_begin fills it)
struct SpRecDev {
    int32_t *cols;             // [n * k] or null: sp_state.active_column of each step, ascending
    int32_t *overlap;          // [n * k] or null: overlaps[active_column]
    double *boosted;           // [n * k] or null: boosted_overlaps[active_column]
    uint32_t base;             // step index of record 0
    int32_t n;                 // records of this call
};

// before the call's first step: one thread
__global__ void k_sp_run_begin(SpRecDev *r, int32_t *cols, int32_t *overlap, double *boosted, uint32_t base, int32_t n) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r->cols = cols;
        r->overlap = overlap;
        r->boosted = boosted;
        r->base = base;
        r->n = n;
    }
}

// r: the descriptor (read by the record blocks only: null in a launch without them)
__global__ __launch_bounds__(256) void k_sp_run_tail(Dev d, const uint32_t *__restrict__ bank, int n_inputs, int p, int n_learn, const SpRecDev *__restrict__ r) {
    const int b = (int)blockIdx.x;
    if (b < n_learn) {
        role_sp_learn_row<true>(d, bank, n_inputs, p, b);
        return;
    }
    const int i = (b - n_learn) * 256 + (int)threadIdx.x;
    const uint32_t slot = d.ctr->step[p] - r->base;
    if (i >= d.k || slot >= (uint32_t)r->n) return;         // (a step outside the call's [base, base + n): nothing is written)
    const int col = d.active_cols[p][i];
    const size_t at = (size_t)slot * d.k + i;
    // (each field's stores of a wave are to consecutive words)
    if (r->cols) r->cols[at] = col;
    if (r->overlap) r->overlap[at] = d.overlap[p][col];
    if (r->boosted) r->boosted[at] = d.boosted[p][col];
}
