// The first launch of the batched run's two-launch step (enqueue_lean, BITHTM_LEAN=2) with the middle role written for the end of
// the launch's longest chain: k_first_handover.  Every other role is called exactly as k_act_mid_rows (htm_pipeline.h) calls it;
// that kernel stays the host-fed step's and the model groups', and process() -- the twin the tests compare run() with -- keeps it.
//
// Block 0 (role_handover_block0).  At the bench shape's steady state no winner is without a segment (n_un == 0 in every traced
// step: profiles/r22_block0_stamps.txt, tools/block0_stamps.py): behind the fan-in the block loads the column lists, stores the
// winner list and the step's counts, and ends -- about 2.3 us for one trip and a handful of stores; none of the allocation below
// runs there.  (Since round 23 not even that: where no activation block raised its flag -- fan_flag, below -- block 0 ends behind
// the wait, and the winner list and the counts are built by the step's last launch, k_last_handover, htm_handover_last.h.  What
// follows is the block where a winner does lack a segment.)  In role_mid's block 0 the compiler places the scalar loads of the kernel's own arguments (Dev is passed by value:
// the list pointers, the output pointers) where a field is first used, behind the wait and behind the lists; here they are read
// before the wait and pinned in registers.  On its own that cannot be told from noise (r22_ab_summary.txt); it is kept because it
// takes loads off the chain and costs nothing.
// While every column bursts (the first steps of a model, a changed input) role_mid's block 0 walks six dependent trips: the lists;
// the ordered lists stored and the stores acknowledged (a __syncthreads for memory); seg_nsyn of the needed 1 024-blocks; the list
// of winners without a segment read back, entry by rank; the new bindings' cells read again; the stores and atomics.  Here:
//   trip 1   the column lists
//            the ordered list of winners without a segment is built in the block's dynamic LDS -- which block 0 never used: the
//            launch asks for SEL_BINS * 4 bytes for the overlap role's histogram on every step
//   trip 2   seg_nsyn AND seg_cell (the owner whose segment count a recycled row leaves) of the first needed 1 024-block, asked
//            for before any store of the block has been issued: gfx9's vmcnt counts loads, stores and atomics in one counter, so a
//            load behind a store waits for the store's acknowledgement whether or not a barrier says so
//   trip 3   every store and atomic of the block: bindings, winners[p], unacc_list (still written: a fork copies it), counters
// Entries of the list beyond the LDS capacity (every column bursting at a large shape; `list_cap`, BITHTM_HANDOVER_LDS_CAP for
// the tests) go through d.unacc_list as before, behind a barrier for memory, and second and later needed 1 024-blocks load
// behind the first one's bindings.  Ranks, lowest-id-first recycling and ascending-cell binding are role_mid's, line by line
// (projections.py:79-95, 271-281).
//
// Classification blocks: role_mid with PRE_NSYN (htm_tm_kernels.h) -- a row's synapse count fetched before the wait.
#ifndef BITHTM_HANDOVER_H
#define BITHTM_HANDOVER_H

// words of the dynamic LDS: [0, HANDOVER_LIST_MAX) the list | HANDOVER_NEED pairs of (1 024-block, first rank) | 256 counts per 2^20 ids
#define HANDOVER_NEED 128
#define HANDOVER_LIST_MAX (SEL_BINS - 2 * HANDOVER_NEED - 256)
static_assert(HANDOVER_LIST_MAX >= 1024, "the dynamic LDS of the launch (SEL_BINS words) holds the list, the needed blocks and the counts");

// diagnostic build (-DBITHTM_HANDOVER_STAMPS, handle created under BITHTM_TRACE=1): block 0's device clock at the ends of its trips,
// and its counts, in the trace rows of the launch slot the two-launch schedule leaves unused (3 + 4 * parity)
#ifdef BITHTM_HANDOVER_STAMPS
#define HSTAMP(i, v) do { if (d.trace && threadIdx.x == 0 && d.ctr->step[p] < d.trace_until) d.trace[(size_t)(3 + 4 * p) * 8192 + (i)] = (v); } while (0)
#else
#define HSTAMP(i, v) do { } while (0)
#endif

template <typename Wait>
__device__ __forceinline__ void role_handover_block0(const Dev &d, int p, int n_active, int learning, int list_cap, uint32_t *dyn, Wait wait) {
    constexpr int BS = 256, LPT = 8;
    Counters *c = d.ctr;
    int *s_un = (int *)dyn, *s_need = (int *)dyn + HANDOVER_LIST_MAX, *s_cnt2 = s_need + 2 * HANDOVER_NEED;
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_cells;
    __shared__ int s_nneed;
    if (threadIdx.x == 0) { s_cells = 0; s_nneed = 0; }
    // (everything the allocation needs of the previous step and of the pool is asked for before the wait: role_mid)
    const int S = c->S, nb = (S + 1023) >> 10;
    const uint32_t recyc_first = (int)threadIdx.x < nb ? (uint32_t)d.recyc_cnt[threadIdx.x] : 0u;
    int n_slots = n_active * d.WPC;
    const int nb2 = (nb + 1023) >> 10;
    const int cnt2_first = (int)threadIdx.x < nb2 ? d.recyc_cnt2[threadIdx.x] : 0;
    const int prev_has_winner = c->has_winner[p ^ 1], prev_n_win = c->n_win[p ^ 1];
    const int has_distal = c->has_distal;
    // ... and the kernel's own arguments.  Dev is passed by value: each of its fields is a scalar load from the argument segment, and
    // the compiler places those where a field is first used -- behind the wait, in front of the list loads, and again in front of the
    // stores.  Pinned to registers here (the empty asm makes the values opaque: they cannot be loaded again later).
    // (as pointers to global memory: behind the asm the compiler no longer sees where they came from, and a generic pointer makes
    // flat loads and stores -- which count as LDS operations too, so that every LDS-only barrier would wait for them)
    typedef __attribute__((address_space(1))) int gint;
    typedef __attribute__((address_space(1))) const u64 gu64c;
    gu64c *actw_id = (gu64c *)d.actw_id, *winw_idx = (gu64c *)d.winw_idx, *unacc_word = (gu64c *)d.unacc_word, *actcnt = (gu64c *)d.actcnt;
    gint *winners = (gint *)d.winners[p], *unacc_list = (gint *)d.unacc_list, *seg_nsyn = (gint *)d.seg_nsyn, *seg_cell = (gint *)d.seg_cell;
    typedef __attribute__((address_space(1))) Counters gctr;
    gctr *ctr = (gctr *)c;
    int match_thr = d.match_thr, Scap = d.Scap;
#ifndef BITHTM_HANDOVER_NO_PIN                      // (a scratch build's switch for measuring this part alone)
    asm volatile("" : "+s"(actw_id), "+s"(winw_idx), "+s"(unacc_word), "+s"(actcnt), "+s"(winners), "+s"(unacc_list), "+s"(seg_nsyn), "+s"(seg_cell),
                      "+s"(match_thr), "+s"(Scap), "+s"(ctr), "+s"(n_slots));
#endif
    c = (Counters *)ctr;
    HSTAMP(0, wall_clock64());
    // Nothing can need a segment (learning off, or no distal state yet: every `unacc` word is 0), or -- behind the wait -- no activation
    // block raised its flag: the block has no binding to make, and the step's winner list and counts are the list role's, one launch
    // later (role_winner_list, htm_handover_last.h, told by n_un == 0).  With learning off the block needs nothing of the activation
    // and does not wait for it.
    auto nothing_to_bind = [&]() {
        if (threadIdx.x == 0) { c->n_un = 0; c->n_bind[p] = 0; }
    };
    if (!learning || !has_distal) { nothing_to_bind(); return; }
    const bool flagged = wait();
    HSTAMP(1, wall_clock64());
    if (!flagged) { HSTAMP(6, 0ull); nothing_to_bind(); return; }
    uint32_t carry_w = 0, carry_u = 0, n_cells = 0;
    // the words of the LAST pass stay in registers: their winners are stored at the end of the block (one pass covers 2 048 words)
    uint32_t ww[LPT];
    int a[LPT];
    uint32_t run_w = 0;
    for (int base = 0; base < n_slots; base += LPT * BS) {
        const int i0 = base + LPT * (int)threadIdx.x;
        uint32_t uw[LPT];
        uint32_t vsum = 0;
        u64 ac = 0;
        if (i0 < n_slots) {                        // (agent-scope loads, 8 bytes each: the arrays are padded by 8 entries)
#pragma unroll
            for (int j = 0; j < LPT; j += 2) {
                const u64 av = __hip_atomic_load(actw_id + ((i0 + j) >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u64 wv = __hip_atomic_load(winw_idx + ((i0 + j) >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const u64 uv = __hip_atomic_load(unacc_word + ((i0 + j) >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a[j] = (int)(uint32_t)av; a[j + 1] = (int)(uint32_t)(av >> 32);
                ww[j] = (uint32_t)wv; ww[j + 1] = (uint32_t)(wv >> 32);
                uw[j] = (uint32_t)uv; uw[j + 1] = (uint32_t)(uv >> 32);
            }
            ac = __hip_atomic_load(actcnt + (i0 >> 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < LPT; ++j) {
                const bool ok = i0 + j < n_slots;
                if (!ok) { ww[j] = 0; uw[j] = 0; }
                n_cells += ok ? (uint32_t)((ac >> (8 * j)) & 0xFFu) : 0u;
            }
        } else {
#pragma unroll
            for (int j = 0; j < LPT; ++j) { a[j] = 0; ww[j] = 0; uw[j] = 0; }
        }
#pragma unroll
        for (int j = 0; j < LPT; ++j) vsum += (uint32_t)__popc(ww[j]) | ((uint32_t)__popc(uw[j]) << 16);    // winners | needing a segment
        uint32_t total;
        const uint32_t run = block_excl_scan<BS, true>(vsum, s_wave, total);
        run_w = carry_w + (run & 0xFFFFu);
        int pu = (int)(carry_u + (run >> 16));
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            uint32_t u1 = uw[j];
            while (u1) {
                const int b = __ffs(u1) - 1;
                u1 &= u1 - 1;
                if (pu < list_cap) s_un[pu] = a[j] * 32 + b; else unacc_list[pu] = a[j] * 32 + b;
                ++pu;
            }
        }
        if (base + LPT * BS < n_slots) {           // (not the last pass: its winners go now)
            int pw = (int)run_w;
#pragma unroll
            for (int j = 0; j < LPT; ++j) {
                uint32_t w1 = ww[j];
                while (w1) { const int b = __ffs(w1) - 1; w1 &= w1 - 1; winners[pw++] = a[j] * 32 + b; }
            }
        }
        carry_w += total & 0xFFFFu;
        carry_u += total >> 16;
    }
    n_cells = wave_sum(n_cells);
    if (lane_id() == 0) atomicAdd(&s_cells, n_cells);
    const int n_un = (learning && has_distal) ? (int)carry_u : 0;
    // what ends the block whichever way it goes: the last pass's winners, the list's copy in memory, the step's counts
    auto finish = [&](int n_r, int n_new, bool bound) {
        int pw = (int)run_w;
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            uint32_t w1 = ww[j];
            while (w1) { const int b = __ffs(w1) - 1; w1 &= w1 - 1; winners[pw++] = a[j] * 32 + b; }
        }
        for (int i = threadIdx.x; i < min((int)carry_u, list_cap); i += BS) unacc_list[i] = s_un[i];
        HSTAMP(8, wall_clock64());
        if (threadIdx.x == 0) {
            c->n_win[p] = (int)carry_w;
            c->has_winner[p] = 1;
            c->n_un = n_un;
            c->n_active_cells = (int)s_cells;
            c->n_bind[p] = bound ? n_r + n_new : 0;
            if (bound) {
                c->n_recycled = n_r;
                c->n_new = n_new;
                c->S_old = S;
                c->S = S + n_new;
            }
        }
    };
    lds_barrier();                                  // (s_cells, the list; LDS only)
    HSTAMP(2, wall_clock64());
    HSTAMP(6, (unsigned long long)n_un);
    if (n_un == 0) { finish(0, 0, false); return; }
    // the needed 1 024-blocks, as role_mid picks them: from the counts in registers where the pool has no more than 256 k ids
    uint32_t carry = 0;                             // recyclable segments seen so far
    for (int r0 = 0; r0 < nb2 && carry < (uint32_t)n_un; r0 += 256) {
        lds_barrier();
        s_cnt2[threadIdx.x] = r0 == 0 ? cnt2_first : (r0 + (int)threadIdx.x < nb2 ? d.recyc_cnt2[r0 + threadIdx.x] : 0);
        lds_barrier();
        for (int r = r0; r < min(r0 + 256, nb2) && carry < (uint32_t)n_un; ++r) {
            if (s_cnt2[r - r0] == 0) continue;
            for (int base = r << 10; base < min(nb, (r + 1) << 10); base += BS) {
                const int b = base + threadIdx.x;
                const uint32_t v = base == 0 ? recyc_first : ((b < nb && b < ((r + 1) << 10)) ? (uint32_t)d.recyc_cnt[b] : 0u);
                uint32_t total;
                const uint32_t ex = block_excl_scan<BS, true>(v, s_wave, total);
                if (v > 0 && carry + ex < (uint32_t)n_un) {
                    const int slot = atomicAdd(&s_nneed, 1);
                    if (slot < HANDOVER_NEED) {
                        s_need[2 * slot] = b;
                        s_need[2 * slot + 1] = (int)(carry + ex);
                    } else {
                        d.recyc_need[2 * slot] = b;
                        d.recyc_need[2 * slot + 1] = (int)(carry + ex);
                    }
                }
                carry += total;
                if (carry >= (uint32_t)n_un) break;
            }
        }
    }
    lds_barrier();
    const int n_need = s_nneed;
    HSTAMP(3, wall_clock64());
    HSTAMP(7, (unsigned long long)n_need);
    // (for memory: list entries beyond the LDS capacity and needed blocks beyond theirs were stored above and are read below)
    if (n_un > list_cap || n_need > HANDOVER_NEED) __syncthreads();
    const int n_r = min(n_un, (int)carry);
    int n_new = n_un - n_r;
    if (S + n_new > Scap) {
        if (threadIdx.x == 0) atomicOr(&c->error, 1);
        n_new = max(Scap - S, 0);
    }
    auto listed = [&](int i) { return i < list_cap ? s_un[i] : unacc_list[i]; };
    // the bound segments are queued from the back of the work array (no reservation to wait for)
    const int wbase = d.work_cap - (n_r + n_new);
    const int n_w = prev_has_winner ? prev_n_win : -1;
    const int grown = n_w > 0 ? min(d.sample, n_w) : 0;
    for (int i = 0; i < n_need; ++i) {              // each needed 1024-block: rank its recyclable segments
        const int b = i < HANDOVER_NEED ? s_need[2 * i] : d.recyc_need[2 * i], off = i < HANDOVER_NEED ? s_need[2 * i + 1] : d.recyc_need[2 * i + 1];
        constexpr int IPT = 1024 / BS;              // consecutive segments per thread
        int owner[IPT];
        uint32_t fl[IPT], cnt = 0;
        // (a row's owner is asked for with its synapse count, whether or not the row turns out to be recycled: one trip, not two)
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int seg = b * 1024 + (int)threadIdx.x * IPT + j, at = min(seg, Scap - 1);
            const bool dead = seg_nsyn[at] < match_thr;
            owner[j] = seg_cell[at];
            fl[j] = (seg < S && dead) ? 1u : 0u;
            cnt += fl[j];
        }
        uint32_t total;
        int rank = off + (int)block_excl_scan<BS, true>(cnt, s_wave, total);
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int seg = b * 1024 + (int)threadIdx.x * IPT + j;
            if (fl[j] && rank < n_r) {              // (tm_bind_segment, the old owner already here)
                const int cell = listed(rank), pos = wbase + rank;
                atomicSub(&d.segcount[owner[j]], 1);
                seg_cell[seg] = cell;
                seg_nsyn[seg] = (int)SEG_BUSY;
                atomicAdd(&d.segcount[cell], 1);
                if (pos < d.work_cap) d.work[pos] = (uint32_t)seg; else atomicOr(&c->error, 4);
            }
            rank += (int)fl[j];
        }
        // the ids recycled out of this 1024-block leave its recyclable count if the learning role is going to grow
        // them past the matching threshold (known now: an empty row grows `grown` synapses) -- one update per block
        if (threadIdx.x == 0 && grown >= d.match_thr) recyc_add(d, b, -max(0, min((int)total, n_r - off)));
    }
    HSTAMP(4, wall_clock64());
    for (int i = threadIdx.x; i < n_new; i += BS) tm_bind_segment(d, S + i, listed(n_r + i), false, wbase + n_r + i);
    if (n_new > 0 && grown < d.match_thr)           // fresh ids [S, S + n_new) that will stay below the matching threshold
        for (int b = (S >> 10) + (int)threadIdx.x; b <= (S + n_new - 1) >> 10; b += BS)
            recyc_add(d, b, min(S + n_new, (b + 1) << 10) - max(S, b << 10));
    finish(n_r, n_new, true);
    HSTAMP(5, wall_clock64());
}

// (a scratch build's switch for measuring the classification blocks' part alone: role_mid, PRE_NSYN)
#ifndef BITHTM_HANDOVER_PRE_NSYN
#define BITHTM_HANDOVER_PRE_NSYN true
#endif

// ---- the flag: "a winner of this step has no segment" -----------------------------------------------------------------------------
// Word 1 of each fan-in counter line (word 0 is the counter fan_wait polls; the lines are 128 bytes apart).  An activation block that
// holds a winner without a segment stores 1 there, agent scope, AHEAD of fan_signal's s_waitcnt vmcnt(0): the store is acknowledged
// before the block counts itself done.  Block 0 reads a line's counter and flag with ONE 8-byte load per lane, so a count that holds
// an arrival comes with that block's flag: it cannot see every arrival and miss a flag.  Reset with the counters by the step's last
// launch (fan_reset_flags, htm_handover_last.h).  At the steady state no block stores anything.
__device__ __forceinline__ uint32_t *fan_line(const Dev &d, int p, int i) { return d.fan + (size_t)(p * FAN_COUNTERS + i) * FAN_STRIDE; }
static_assert(FAN_STRIDE >= 2 && (FAN_STRIDE * 4) % 8 == 0, "a line holds the counter and the flag, 8 bytes aligned");

__device__ __forceinline__ void fan_flag(const Dev &d, int p, int b, bool raise) {
    if (__ballot(raise) != 0 && lane_id() == 0)
        __hip_atomic_store(fan_line(d, p, b & (FAN_COUNTERS - 1)) + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// fan_wait (htm_pipeline.h: the same bounded spin, error bit 32) that also tells whether any arrived block raised its flag
__device__ __forceinline__ bool fan_wait_flagged(const Dev &d, int p, uint32_t target) {
    __shared__ uint32_t s_flagged;
    if (threadIdx.x < 64) {
        u64 flags = 0;
        for (int looks = 0;; ++looks) {
            const u64 v = threadIdx.x < FAN_COUNTERS
                              ? __hip_atomic_load((const u64 *)fan_line(d, p, (int)threadIdx.x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            flags = __ballot((uint32_t)(v >> 32) != 0u);
            if (wave_sum((uint32_t)v) >= target) break;
            if (looks >= (1 << 18)) {                                // (an activation block never arrived)
                if (threadIdx.x == 0) atomicOr(&d.ctr->error, 32);
                break;
            }
            __builtin_amdgcn_s_sleep(BITHTM_FAN_SLEEP);
        }
        if (threadIdx.x == 0) s_flagged = flags != 0 ? 1u : 0u;
    }
    __syncthreads();
    return s_flagged != 0u;
}

// role_activate<true> (htm_sp_kernels.h), returning whether the lane group's column has a winner without a segment
__device__ __forceinline__ bool role_activate_unacc(const Dev &d, int p, int blk, int n_active) {
    const int idx = blk * tm_groups_per_block(d) + tm_group_of(d, threadIdx.x);
    const bool ok = idx < n_active;
    const int a = ok ? d.active_cols[p][idx] : 0;
    const ColumnWords w = tm_column_words(d, p, 1, ok, a, tm_pred_words(d, p, ok, a));
    tm_store_column<true>(d, p, ok, a, idx, w);
    return ok && w.unacc != 0;
}

// grid and arguments: k_act_mid_rows' (htm_pipeline.h); list_cap: entries of the list of winners without a segment kept in LDS
__global__ __launch_bounds__(256, BITHTM_LEAN2_WAVES) void k_first_handover(Dev d, int p, int n_active, int n_act_blocks, int learning, int n_cls,
                                                        const uint32_t *__restrict__ bank, int n_inputs, int n_rows, int G, int n_overlap_blocks,
                                                        int n_duty_blocks, int n_clear_blocks, int order, int list_cap) {
    TraceScope ts(d, 0 + 4 * p);
    int b = blockIdx.x;
    int role = 4;
#pragma unroll
    for (int i = 3; i >= 0 && role == 4; --i) {
        const int r = (order >> (4 * i)) & 15;
        const int n = r == 0 ? n_act_blocks : r == 1 ? 1 + n_cls : r == 2 ? n_rows : n_overlap_blocks;
        if (b < n) role = r; else b -= n;
    }
    if (role == 0) {
        fan_flag(d, p, b, role_activate_unacc(d, p, b, n_active));
        fan_signal(d, p, b);
        return;
    }
    if (role == 1) {
        auto wait = [&]() { fan_wait(d, p, (uint32_t)n_act_blocks); };
        if (b == 0) role_handover_block0(d, p, n_active, learning, list_cap, (uint32_t *)dyn_lds, [&]() { return fan_wait_flagged(d, p, (uint32_t)n_act_blocks); });
        else { __builtin_assume(b > 0); role_mid<256, decltype(wait), BITHTM_HANDOVER_PRE_NSYN>(d, p, n_active, 1, learning, b, n_cls, 1, wait); }   // (role_mid's own block 0 is not this kernel's)
        return;
    }
    if (role == 2) {
        if (n_overlap_blocks > 0) role_sp_row<256, true>(d, p, bank, n_inputs, 0, b, threadIdx.x);
        else role_sp_row<256>(d, p, bank, n_inputs, 0, b, threadIdx.x);
        return;
    }
    if (role == 3) {
        if (d.planes) role_overlap_planes(d, bank, n_inputs, p, p ^ 1, 1, b, n_overlap_blocks, (uint32_t *)dyn_lds, n_rows > 0 ? 2 : 1);
        else role_overlap<256>(d, bank, n_inputs, G, p, p ^ 1, 1, b, n_overlap_blocks, (uint32_t *)dyn_lds, 1, n_rows > 0 ? 2 : 1);
        return;
    }
    if (b < n_duty_blocks) {
        role_duty(d, p, b, 0, d.C);
        return;
    }
    b -= n_duty_blocks;
    if (b < n_clear_blocks) {
        role_clear_dense(d, p, b, n_clear_blocks);
        return;
    }
    role_zero_match(d, p, b - n_clear_blocks, (int)gridDim.x - n_act_blocks - 1 - n_cls - n_rows - n_overlap_blocks - n_duty_blocks - n_clear_blocks, d.ctr->S);
}

#endif
