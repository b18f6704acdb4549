// The last launch of the batched run's two-launch step (enqueue_lean, BITHTM_LEAN=2) -- the launch behind k_first_handover
// (htm_handover.h): k_learn_scan_emit (htm_pipeline.h), its roles called exactly as that kernel calls them, and one block more at the
// end of the grid, the list role.  Every other schedule keeps k_learn_scan_emit.
//
// The list role (role_winner_list).  The step's ordered winner list, n_win[p], has_winner[p] and n_active_cells are read by nothing in
// the step that writes them: this launch's learning role reads the PREVIOUS step's list (winners[p ^ 1], n_win[p ^ 1]), the next
// step's block 0 reads n_win[p ^ 1] behind this launch, and the record, capture, decode, feedback, reset, fork, view, info and read
// paths all run behind the step's last launch.  In k_first_handover they stood at the end of the launch's longest chain -- block 0:
// fan-in, one trip for the column lists, the stores.  Where no winner of the step lacks a segment (n_un == 0, stored by block 0 a
// launch earlier: every traced steady-state step of the bench shape) block 0 now ends behind its wait and the list is built here,
// where the activation's words lie behind a kernel boundary: plain loads, no fan-in -- 4.5 us of one block, from 3.1 us on, under a
// launch of 8 to 9 (profiles/r23_step_spans.txt).
// Where a winner does lack a segment (n_un > 0) block 0 needs the lists for its bindings anyway, writes the winner list and the
// counts as before, and this role does nothing.
// Nothing in the launch waits for the list block.  It is the grid's last block: the emit blocks still come first, all resident.
// It also resets the fan-in counters (as k_learn_scan_emit's last block does) and the flag words beside them.
#ifndef BITHTM_HANDOVER_LAST_H
#define BITHTM_HANDOVER_LAST_H

// the counters AND the flags of the step's first launch (fan_flag, htm_handover.h), by the list block -- the grid's last, as in
// fan_reset: the other blocks do not even look
__device__ __forceinline__ void fan_reset_flags(const Dev &d, int p) {
    if (threadIdx.x < FAN_COUNTERS) *(u64 *)fan_line(d, p, (int)threadIdx.x) = 0ull;
}

// The list pass of role_handover_block0 without its unaccounted half: one block, 2 048 slots per pass.  Its block-wide scratch (the
// waves' totals, the cell count) lies in the launch's dynamic LDS, which a block of this role has to itself: no static LDS is added.
__device__ __forceinline__ void role_winner_list(const Dev &d, int p, uint32_t *dyn) {
    constexpr int BS = 256, LPT = 8;
    Counters *c = d.ctr;
    if (c->n_un != 0) return;                       // (block 0 of the first launch bound segments: the list and the counts are its)
    uint32_t *s_wave = dyn, *s_cells = dyn + 16;
    if (threadIdx.x == 0) *s_cells = 0;
    const int n_slots = d.k * d.WPC;
    const u64 *actw_id = (const u64 *)d.actw_id, *winw_idx = (const u64 *)d.winw_idx, *actcnt = (const u64 *)d.actcnt;
    int *winners = d.winners[p];
    uint32_t carry_w = 0, n_cells = 0;
    for (int base = 0; base < n_slots; base += LPT * BS) {
        const int i0 = base + LPT * (int)threadIdx.x;
        uint32_t ww[LPT];
        int a[LPT];
        uint32_t vsum = 0;
        if (i0 < n_slots) {                         // (8 bytes each: the arrays are padded by 8 entries)
#pragma unroll
            for (int j = 0; j < LPT; j += 2) {
                const u64 av = actw_id[(i0 + j) >> 1], wv = winw_idx[(i0 + j) >> 1];
                a[j] = (int)(uint32_t)av; a[j + 1] = (int)(uint32_t)(av >> 32);
                ww[j] = (uint32_t)wv; ww[j + 1] = (uint32_t)(wv >> 32);
            }
            const u64 ac = actcnt[i0 >> 3];
#pragma unroll
            for (int j = 0; j < LPT; ++j) {
                const bool ok = i0 + j < n_slots;
                if (!ok) ww[j] = 0;
                n_cells += ok ? (uint32_t)((ac >> (8 * j)) & 0xFFu) : 0u;
                vsum += (uint32_t)__popc(ww[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < LPT; ++j) { a[j] = 0; ww[j] = 0; }
        }
        uint32_t total;
        int pw = (int)(carry_w + block_excl_scan<BS, true>(vsum, s_wave, total));
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            uint32_t w1 = ww[j];
            while (w1) { const int b = __ffs(w1) - 1; w1 &= w1 - 1; winners[pw++] = a[j] * 32 + b; }
        }
        carry_w += total;
    }
    n_cells = wave_sum(n_cells);
    if (lane_id() == 0) atomicAdd(s_cells, n_cells);
    lds_barrier();
    if (threadIdx.x == 0) {
        c->n_win[p] = (int)carry_w;
        c->has_winner[p] = 1;
        c->n_active_cells = (int)*s_cells;
    }
}

// grid: [emit][learning][scan][the list block]; template parameters, arguments and forms: k_learn_scan_emit's
template <int EPL, int MINW, bool TAB = false>
__global__ __launch_bounds__(256, MINW) void k_last_handover(Dev d, int p, int n_emit_blocks, int n_learn_blocks, int n_scan_blocks, int n_spec) {
    TraceScope ts(d, 2 + 4 * p);
    constexpr bool LARGE = MINW < 6;
    static_assert(!(LARGE && TAB), "the streaming scan reads the cell words from memory");
    const bool dyn = LARGE && n_scan_blocks > 0;
    if (n_scan_blocks < 0) n_scan_blocks = -n_scan_blocks;
    int b = blockIdx.x, scan_blk;
    if (b < n_emit_blocks) {
        role_emit(d, p ^ 1, 1, 1, 0, b, n_emit_blocks, (EmitShared *)dyn_lds, 1);
        if (!dyn) return;
        scan_blk = -1 - b;                           // (joins the scan)
    } else if (b < n_emit_blocks + n_learn_blocks) {
        role_learn<EPL, 256, true>(d, p, b - n_emit_blocks, n_learn_blocks, (LearnShared<EPL, 256> *)dyn_lds);
        if (!dyn) return;
        scan_blk = -1 - b;
    } else {
        scan_blk = b - n_emit_blocks - n_learn_blocks;
        if (__builtin_expect(scan_blk == n_scan_blocks, 0)) {      // (the block behind the scan's, the grid's last)
            fan_reset_flags(d, p);
            role_winner_list(d, p, (uint32_t *)dyn_lds);
            return;
        }
    }
    if (LARGE) {
        role_scan<256, true, true, false, true>(d, p, scan_blk, n_scan_blocks, dyn ? n_emit_blocks + n_learn_blocks : 0, (uint32_t *)dyn_lds);
    } else {
        role_scan<256, true, false, TAB>(d, p, scan_blk, n_scan_blocks, n_spec, (uint32_t *)dyn_lds);
    }
}

#endif
