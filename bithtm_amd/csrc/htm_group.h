// Model groups (htm_group_create / htm_group_run, include/bithtm_hip.h): B independent models of one shape stepped by ONE
// launch sequence.  Every launch covers all B members: the grid's y dimension is the member index, and a member's blocks read
// its device state through a table of descriptors (tab[blockIdx.y]: the member's own Dev, with sel_passes = all launched
// digits) -- the same role functions as the solo kernels, with the same blockIdx.x / gridDim.x.
//
// The schedule is the one-role-per-launch, non-fused one of enqueue_rest:
//   kgrp_overlap   role_overlap, top key digit                   (k_sp_overlap, wmode 0)
//   kgrp_select    role_sel_pass, one per further digit          (k_sel_pass)
//   kgrp_count     per-256-column counts above / at the k-th key (k_sp_count)
//   kgrp_emit      role_emit, fused = 0, EMIT_ALL                (k_sp_emit)
//   kgrp_middle    role_mid + the permanence rows if they do not ride in the tail (k_mid_rows, rows_ahead 0, no duty blocks)
//   kgrp_tail      role_learn + role_scan + the permanence rows   (k_learn_scan_tail, n_rows = k or 0)
//     or kgrp_learn + kgrp_scan for pools whose scan streams   (k_tm_learn + k_tm_scan)
//   kgrp_rec_step  the per-step record                            (k_rec_step), kgrp_rec_clear + kgrp_rec_begin before a recorded call
// No block of these launches waits for another block: a grid of B x blocks is not resident at once and dispatch order is
// undefined.  The in-kernel select finish (role_emit with fused != 0), the windowed select (wmode, which needs it), the record
// exchange of shards and the fan-in of k_act_mid_rows (fan_wait) are the only spin loops of the roles, and none is reachable
// from here: fused and wmode are compile-time zeros below, role_mid gets its NoWait default, and nothing is sharded.
// Part of the single translation unit htm_engine.hip (included after htm_record.h).
#ifndef BITHTM_HTM_GROUP_H
#define BITHTM_HTM_GROUP_H

// a member's record buffers (kgrp_rec_begin): the pointers k_rec_begin takes as arguments
struct GrpRecArgs {
    htm_step_record *rec;
    int32_t *cols;
    uint32_t *colpred;
};

__global__ __launch_bounds__(RB) void kgrp_overlap(const Dev *__restrict__ tab, const uint32_t *const *__restrict__ banks, int n_inputs,
                                                   int G, int p) {
    __shared__ uint32_t h[SEL_BINS];
    const Dev &d = tab[blockIdx.y];
    role_overlap<RB>(d, banks[blockIdx.y], n_inputs, G, p, p, 0, blockIdx.x, gridDim.x, h, 0);
}

__global__ __launch_bounds__(RB) void kgrp_select(const Dev *__restrict__ tab, int pass, int sp) {
    __shared__ SelShared sh;
    const Dev &d = tab[blockIdx.y];
    role_sel_pass<RB>(d, pass, sp, blockIdx.x, gridDim.x, &sh);
}

__global__ __launch_bounds__(256) void kgrp_count(const Dev *__restrict__ tab, int sp) { role_sp_count(tab[blockIdx.y], sp); }

__global__ __launch_bounds__(256) void kgrp_emit(const Dev *__restrict__ tab, int p) {
    __shared__ EmitShared sh;
    const Dev &d = tab[blockIdx.y];
    role_emit(d, p, 1, 0, EMIT_ALL, blockIdx.x, gridDim.x, &sh, 0);
}

// blocks [0, 1 + n_cls): the middle of the TM step; then n_rows permanence rows of this step; the rest zero the match bits
__global__ __launch_bounds__(256, BITHTM_MID_ROWS_WAVES) void kgrp_middle(const Dev *__restrict__ tab, int p, int learning, int n_cls,
                                                                          const uint32_t *const *__restrict__ banks, int n_inputs, int n_rows) {
    const Dev &d = tab[blockIdx.y];
    int b = blockIdx.x;
    if (b <= n_cls) {
        role_mid<256>(d, p, d.k, 1, learning, b, n_cls);
        return;
    }
    b -= 1 + n_cls;
    if (b < n_rows) {
        role_sp_row<256, false, true, false>(d, p, banks[blockIdx.y], n_inputs, 0, b, threadIdx.x);     // (HOLD off: the launch's scratch)
        return;
    }
    b -= n_rows;
    role_zero_match(d, p, b, (int)gridDim.x - 1 - n_cls - n_rows, d.ctr->S);
}

// the learning role, the scan and (n_rows > 0) this step's permanence rows: k_learn_scan_tail without the shard's overlap
template <int EPL>
__global__ __launch_bounds__(256, 6) void kgrp_tail(const Dev *__restrict__ tab, int p, int n_learn_blocks, int n_scan_blocks, int n_spec,
                                                    const uint32_t *const *__restrict__ banks, int n_inputs) {
    const Dev &d = tab[blockIdx.y];
    int b = blockIdx.x;
    fan_reset(d, p);
    if (b < n_learn_blocks) {
        role_learn<EPL, 256, true>(d, p, b, n_learn_blocks, (LearnShared<EPL, 256> *)dyn_lds);
        return;
    }
    b -= n_learn_blocks;
    if (b < n_scan_blocks) {
        role_scan<256, true, false, false>(d, p, b, n_scan_blocks, n_spec, (uint32_t *)dyn_lds);
        return;
    }
    role_sp_row<256>(d, p, banks[blockIdx.y], n_inputs, 0, b - n_scan_blocks, threadIdx.x);
}

// pools whose scan streams (or whose column bitmap does not fit the LDS beside it): the two roles in launches of their own
// (7 waves per SIMD, as k_tm_learn<1..4> has: without the bound the table's address took the role to 77 VGPRs and 6 waves)
template <int EPL>
__global__ __launch_bounds__(RB, 7) void kgrp_learn(const Dev *__restrict__ tab, int p) {
    const Dev &d = tab[blockIdx.y];
    fan_reset(d, p);
    role_learn<EPL, RB>(d, p, blockIdx.x, gridDim.x, (LearnShared<EPL, RB> *)dyn_lds);
}

template <bool use_lds, int MINW>
__global__ __launch_bounds__(256, MINW) void kgrp_scan(const Dev *__restrict__ tab, int p, int n_spec) {
    const Dev &d = tab[blockIdx.y];
    role_scan<256, use_lds, MINW == 1>(d, p, blockIdx.x, gridDim.x, n_spec, (uint32_t *)dyn_lds);
}

// records: every member's descriptor zeroed, then filled (one block per member), then one record launch behind each step
__global__ __launch_bounds__(64) void kgrp_rec_clear(RecDev *const *__restrict__ recs) {
    uint32_t *w = (uint32_t *)recs[blockIdx.x];
    for (int i = threadIdx.x; i < (int)(sizeof(RecDev) / 4); i += 64) w[i] = 0u;
}

// (record 0 is the member's next step: the index the last completed step -- parity q -- left in the counter block)
__global__ __launch_bounds__(256) void kgrp_rec_begin(const Dev *__restrict__ tab, int q, RecDev *const *__restrict__ recs,
                                                      const GrpRecArgs *__restrict__ args, int32_t n) {
    const Dev &d = tab[blockIdx.y];
    const GrpRecArgs &a = args[blockIdx.y];
    role_rec_begin(d, q, recs[blockIdx.y], a.rec, a.cols, a.colpred, d.ctr->step[q ^ 1], n);
}

__global__ __launch_bounds__(256) void kgrp_rec_step(const Dev *__restrict__ tab, int p, RecDev *const *__restrict__ recs) {
    role_rec_step(tab[blockIdx.y], p, recs[blockIdx.y], tab[blockIdx.y].k);
}

// ------------------------------------------------------------------------------------------
// Inference views (htm_create_view): a group whose members all alias ONE segment store, stepped without
// learning.  kgrp_scan replaces nothing of the store between its members' scans, yet reads every row once per member; this scan
// reads each row once per chunk of M members (grid y = chunk).  The block stages the M members' column bitmaps in LDS (colwords
// words each, M * colwords * 4 <= 64 KiB), and each wave takes groups of 16 rows as role_scan does (8 lanes per row, two rows
// per lane group, 4 synapses per lane and chunk of 32).  Every chunk of a row is loaded ONCE; for each member the wave tests
// the chunk's synapses against that member's bitmap, gathers that member's active-cell words for the hits and adds potential
// and connected counts (the connected flag is presyn bit 31, as the solo scan reads it) into the member's own accumulators
// (registers: GRP_SHARED_MMAX x 2 per lane).  A matching row is then published into each member's own buffers with the
// member's own jitter key (its step index) -- seg_info, seg_jit, match bits, per-cell maxima, prediction bits -- exactly
// what role_scan publishes, so the members end bit-identical to their per-member scans (only the order of the atomics
// differs, and atomicMax / atomicOr do not depend on it).  Block 0 does role_scan's counter housekeeping for each member.
//
// Not carried over from role_scan: the speculative first batch (n_spec -- the loads of a block's first rows before the segment
// count arrives: one round trip per block, and this grid is only the blocks resident at once, each streaming many groups), the
// early-out of rows that cannot match (per member it would need the hit counts of every member before any gather -- the gathers
// are of hits only, most rows have few), and the LDS tables of the three-launch schedule.  Rows on a learning role's work list
// (SEG_BUSY) are skipped as role_scan skips them; with learning = 0 there are none.
// The members' learning role (kgrp_learn, learning = 0) runs before this launch: it clears the previous scan's maxima.
#define GRP_SHARED_MMAX 16

__global__ __launch_bounds__(256) void kgrp_scan_shared(const Dev *__restrict__ tab, int B, int M, int p) {
    const int m0 = (int)blockIdx.y * M, nm = min(M, B - m0);
    const Dev &d = tab[m0];                          // (the store: the same rows in every member's descriptor)
    const int cw = d.colwords, lk = d.LK;
    uint32_t *s_bits = (uint32_t *)dyn_lds;          // [nm][cw]
    for (int m = 0; m < nm; ++m) {
        const uint32_t *src = tab[m0 + m].colbits[p];
        for (int i = threadIdx.x; i < cw; i += 256) s_bits[m * cw + i] = src[i];
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < nm) {  // role_scan's housekeeping, member by member
        Counters *c = tab[m0 + (int)threadIdx.x].ctr;
        c->step[p ^ 1] = c->step[p] + 1;
        c->has_distal = 1;
        c->n_work[p ^ 1] = 0;
        c->n_bind[p ^ 1] = 0;
    }
    __syncthreads();
    const int S = d.ctr->S;                          // (equal in every member: copied from the parent by each call)
    const int wave = threadIdx.x >> 6, gi = (threadIdx.x & 63) >> 3, l = threadIdx.x & 7;
    const int n_waves = (int)gridDim.x * 4;
    for (int g = (int)blockIdx.x * 4 + wave; g * 16 < S; g += n_waves) {
        int seg[2], n[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            seg[u] = g * 16 + u * 8 + gi;
            const int nn = seg[u] < S ? d.seg_nsyn[seg[u]] : 0;
            n[u] = (nn & (int)SEG_BUSY) ? 0 : nn;
        }
        uint32_t acc[GRP_SHARED_MMAX][2];
#pragma unroll
        for (int m = 0; m < GRP_SHARED_MMAX; ++m) acc[m][0] = acc[m][1] = 0u;
        for (int c = 0; __any(n[0] > c * 32 || n[1] > c * 32); ++c) {
            uint32_t e[8], valid = 0u;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int4 v = make_int4(0, 0, 0, 0);
                if (n[u] > c * 32) v = *(const int4 *)(d.presyn + (size_t)seg[u] * d.E + c * 32 + l * 4);
                const int nv = min(max(n[u] - c * 32 - l * 4, 0), 4);
                valid |= ((1u << nv) - 1u) << (4 * u);
                e[4 * u] = (uint32_t)v.x; e[4 * u + 1] = (uint32_t)v.y; e[4 * u + 2] = (uint32_t)v.z; e[4 * u + 3] = (uint32_t)v.w;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) e[i] = ((valid >> i) & 1u) ? e[i] : 0u;     // (a slot past the row's count names nothing)
#pragma unroll
            for (int m = 0; m < GRP_SHARED_MMAX; ++m) {
                if (m < nm) {                        // (block-uniform)
                    const uint32_t *bits = s_bits + m * cw;
                    uint32_t hit = 0u;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t w = bits[(e[i] & SYN_CELL) >> (lk + 5)];
                        hit |= ((w >> ((e[i] >> lk) & 31)) & 1u) << i;
                    }
                    hit &= valid;
                    if (hit) {
                        const uint32_t *act = tab[m0 + m].act[p];
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            if ((hit >> i) & 1u) {
                                const uint32_t a = (act[(e[i] & SYN_CELL) >> 5] >> (e[i] & 31)) & 1u;
                                acc[m][i >> 2] += a + ((a & (e[i] >> 31)) << 16);     // potential (:247) | connected-active << 16 (:171-172)
                            }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 0; m < GRP_SHARED_MMAX; ++m) {
            if (m < nm) {
                const Dev &dm = tab[m0 + m];
                bool matching[2];
                int pot[2], conn[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const uint32_t sum = (uint32_t)group8_sum_first((int)acc[m][u]);      // (valid in the row's first lane only)
                    pot[u] = (int)(sum & 0xFFFFu);
                    conn[u] = (int)(sum >> 16);
                    matching[u] = l == 0 && seg[u] < S && pot[u] >= dm.match_thr;        // :247
                }
                if (__any(matching[0] || matching[1])) {
                    const uint32_t base3 = htm_stream_base(dm.seed, HTM_STREAM_SEGMENT_JITTER, dm.ctr->step[p]);
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        if (matching[u]) {
                            const int cell = d.seg_cell[seg[u]];
                            const float jit = htm_jitter((float)pot[u], htm_draw24(base3, (uint32_t)seg[u], 0u));   // :234-235
                            const bool active = conn[u] >= dm.act_thr;                       // :250
                            atomicMax(&dm.cellmax[p][cell], __float_as_uint(jit));          // :237
                            if (active) atomicOr(&dm.pred[p][cell >> 5], 1u << (cell & 31));   // :251
                            dm.seg_info[seg[u]] = (uint32_t)pot[u] | ((uint32_t)conn[u] << 12) | 0x40000000u | (active ? 0x80000000u : 0u);
                            dm.seg_jit[seg[u]] = jit;
                        }
                }
                const u64 b0 = __ballot(matching[0]), b1 = __ballot(matching[1]);      // (role_scan's gathering of the 16 bits)
                const uint32_t bits = (uint32_t)(((b0 & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) |
                                      ((uint32_t)(((b1 & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << 8);
                if ((threadIdx.x & 63) == 0 && bits) atomicOr(&dm.match_bits[p][g >> 1], bits << (16 * (g & 1)));
            }
        }
    }
}

#endif
