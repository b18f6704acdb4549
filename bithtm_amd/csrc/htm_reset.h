// Sequence resets (htm_reset, htm_set_run_resets; include/bithtm_hip.h).
//
// A reset before step t makes step t run as the reference does after `tm.last_state = tm.get_empty_state()`
// (networks.py:57-65,91-93): no predictions (every active column bursts), distal_state None (no best-matching cells, no
// distal_projection.update: projections.py:257-259), winner_cell None.  The device state this leaves is the one
// htm_import_commit leaves after importing get_empty_state(): the previous step's prediction, activation and winner words
// and its winner list cleared, has_winner / has_distal 0, no matching segment (info words, jitter, match bits of both
// parities), the coming scan's per-cell maxima clean, and the learning role of step t told to clear ALL of the previous
// scan's maxima (cm_dense_step), since has_distal no longer tells it how many rows the sparse clear would need.  The
// segment store, the Spatial Pooler, the step index, epsilon and the sticky capacity flags stay what they are.
//
// Inside htm_run the launch goes before the step's activation role (enqueue_rest: after the previous step's scan, which
// every schedule ends a step with), reads the step index from the counter block and returns at once unless the bank row
// of the step has its reset bit set.  It is only enqueued (and captured) in runs that have reset bits.

// device-side descriptor of the reset bits of the current run (one per handle; graphs hold its address, each call with
// resets fills it before its first step)
struct ResetDev {
    const uint32_t *bits;      // [ceil(n / 32)] bit r: reset before every step that reads bank row r
    int32_t n;                 // rows of the bank
    int32_t pad;
};

__global__ __launch_bounds__(64) void k_reset_begin(ResetDev *r, const uint32_t *bits, int32_t n) {
    if (threadIdx.x == 0) { r->bits = bits; r->n = n; }
}

// The reset itself, before the step of parity p (the previous step's buffers are p ^ 1), grid-stride over blockIdx.x: `step` is
// the coming step's index; rec: the recorded call's descriptor, or null: its "predicted before" becomes 0.  (A role of its own:
// the masked reset of a model group's live tick, htm_live.h, calls it per member.)
__device__ __forceinline__ void role_tm_reset(const Dev &d, int p, RecDev *rec, uint32_t step) {
    Counters *c = d.ctr;
    const int q = p ^ 1;
    const int i0 = (int)(blockIdx.x * 256 + threadIdx.x), stride = (int)gridDim.x * 256;
    const int S = d.world > 1 ? c->L : c->S;
    for (int i = i0; i < d.C * d.WPC; i += stride) { d.act[q][i] = 0u; d.pred[q][i] = 0u; d.win[q][i] = 0u; }
    for (int i = i0; i < S; i += stride) { d.seg_info[i] = 0u; d.seg_jit[i] = 0.f; }
    for (int i = i0; i < (d.Lcap + 255) / 256 * 8; i += stride) { d.match_bits[0][i] = 0u; d.match_bits[1][i] = 0u; }
    for (int i = i0; i < d.C * d.KP; i += stride) d.cellmax[p][i] = 0u;
    for (int i = i0; i < d.k; i += stride) d.active_cols[q][i] = 0;
    if (i0 == 0) {
        c->n_win[q] = 0;
        c->has_winner[q] = 0;
        c->has_distal = 0;
        c->cm_dense_step = step + 1u;
        if (rec) rec->prev_pred = 0;
    }
}

// p: parity of the step the reset goes before.  rd: the run's reset bits, or null (htm_reset: unconditional, `step` is the
// coming step's index).  rec: as role_tm_reset takes it.
__global__ __launch_bounds__(256) void k_tm_reset(Dev d, int p, const ResetDev *rd, RecDev *rec, uint32_t step) {
    if (rd) {
        step = d.ctr->step[p];
        const uint32_t row = step % (uint32_t)rd->n;
        if (!((rd->bits[row >> 5] >> (row & 31)) & 1u)) return;      // (the same answer in every block)
    }
    role_tm_reset(d, p, rec, step);
}
