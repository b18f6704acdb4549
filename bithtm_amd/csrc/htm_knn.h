// KNN classifier on the device (htm_knn_*, include/bithtm_hip.h; the definition is bithtm_amd/knn.py, which
// this file equals bit for bit).  One object keeps the store -- `capacity` slots of max_pairs (index, word) pairs each (unused pairs
// (-1, 0)), a label (int32) and a stamp (int64: the object's step total at the step that stored the slot) per slot -- and the
// scratch of an update: the overlaps of a chunk of query steps with every slot, 16 bits each (max_pairs <= 2047: an overlap is at
// most 32 * max_pairs), and, for tables too large for LDS, the chunk's dense query tables.  The slots in use and the step total are
// the host's: every store is decided by what the host knows.
//
// An update over n steps' patterns is, per call,
//   kknn_place     one block: the slot of every labelled step of the call -- count plus the prefix sum over the call's label flags --
//   kknn_append    a thread per pair, 8 bytes each: the labelled steps' patterns into their slots, with label and stamp
// (both only when the call stores anything) and then per chunk of HTM_KNN_CHUNK query steps
//   kknn_distance_lds     grid (slot blocks, query groups): a block stages the dense word tables of its group's queries in LDS
//                  (cleared, then scattered from the queries' pairs), streams its HTM_KNN_SLOTS slots' pairs once -- a thread per
//                  pair, 8 bytes, coalesced -- and looks every pair's word up in each staged table: popcount(word & table[index])
//                  into the (query, slot) sum in LDS; then the sums go out as 16-bit overlaps, 0 where the slot's stamp is not
//                  below the query's step total (a step never sees itself or later steps of its call)
//   kknn_select    a block per query: the histogram of its candidates' overlaps (>= min_overlap) gives the k-th overlap (in two
//                  levels where the overlaps outnumber the bins), a walk in slot order takes everything above it and the lowest
//                  slots at it, votes per label in LDS, the result row (and the votes row)
// and, where one table does not fit HTM_KNN_TABLE_BYTES of LDS, kknn_distance_global between kknn_scatter (the queries' tables into
// the global scratch table) and kknn_scatter again (the same words zeroed: the table is zero between chunks).  There a block stages a
// presence bitmap of each of its queries in LDS -- a bit per table word, while one bitmap fits the same budget -- and goes to the global
// table only for the pairs whose word the query holds: a query holds a few per cent of the words, and the 4-byte gathers were the cost.  No block waits for
// another, nothing is accumulated across blocks, every sum is an integer.  The arithmetic is in the __host__ __device__ functions at
// the top: tests/host_stub/knn_host.cpp evaluates them on the host.
// Every kernel's body is a __device__ function (knn_place_block, knn_append_pair, knn_scatter_pair, knn_distance_block,
// knn_select_block): htm_knn_bank.h calls the same bodies with a member's offsets.
// Part of the single translation unit htm_engine.hip (included after htm_classifier.h, whose pairs and live bits it shares).
#ifndef BITHTM_HTM_KNN_H
#define BITHTM_HTM_KNN_H

#include <stdint.h>

#include "htm_classifier.h"

#define HTM_KNN_CHUNK 64                    // query steps per launch (bithtm_amd/_lib.py: KNN_CHUNK)
#define HTM_KNN_SLOTS 256                   // slots per block of the distance launch (KNN_SLOTS)
#define HTM_KNN_QUERIES 8                   // queries a block stages at most (KNN_QUERIES)
#define HTM_KNN_TABLE_BYTES (48 * 1024)     // LDS for the staged tables of a block (KNN_TABLE_BYTES); with the sums: 56 KiB
#define HTM_KNN_BINS 2048                   // bins of the select's histogram (KNN_BINS)
#define HTM_KNN_MAX_LABELS 1024
#define HTM_KNN_MAX_K 64
#define HTM_KNN_MAX_CAPACITY (1 << 20)
#define HTM_KNN_MAX_PAIRS 2047

// the bits two words share
CLS_HD static inline int knn_pair_overlap(uint32_t a, uint32_t b) { return __builtin_popcount(a & b); }

// words of one dense query table: C * WPC
CLS_HD static inline int64_t knn_table_words(int n_cols, int WPC) { return (int64_t)n_cols * WPC; }
// 1: the tables of a block's queries lie in LDS; 0: in the global scratch table
CLS_HD static inline int knn_in_lds(int64_t words) { return words * 4 <= HTM_KNN_TABLE_BYTES; }
// words of one query's presence bitmap in the global-table form: a bit per table word
CLS_HD static inline int64_t knn_bitmap_words(int64_t words) { return (words + 31) / 32; }
// 1: the blocks of the global-table form stage their queries' presence bitmaps in LDS (one bitmap fits the budget)
CLS_HD static inline int knn_has_bitmap(int64_t words) { return !knn_in_lds(words) && knn_bitmap_words(words) * 4 <= HTM_KNN_TABLE_BYTES; }
// queries a block of the distance launch stages: the tables, or the bitmaps, that fit the budget
CLS_HD static inline int knn_queries(int64_t words) {
    if (!knn_in_lds(words) && !knn_has_bitmap(words)) return HTM_KNN_QUERIES;
    const int64_t fit = HTM_KNN_TABLE_BYTES / ((knn_in_lds(words) ? words : knn_bitmap_words(words)) * 4);
    return (int)(fit < HTM_KNN_QUERIES ? fit : HTM_KNN_QUERIES);
}
// dynamic LDS of a block of the distance launch, in bytes
CLS_HD static inline int64_t knn_distance_lds(int64_t words) {
    return knn_in_lds(words) ? knn_queries(words) * words * 4 : knn_has_bitmap(words) ? knn_queries(words) * knn_bitmap_words(words) * 4 : 0;
}
// blocks along x of the distance launch over `count` slots, and block b's slots [first, last)
CLS_HD static inline int knn_slot_blocks(int count) { return (count + HTM_KNN_SLOTS - 1) / HTM_KNN_SLOTS; }
CLS_HD static inline int knn_block_first(int b) { return b * HTM_KNN_SLOTS; }
CLS_HD static inline int knn_block_last(int b, int count) { return (b + 1) * HTM_KNN_SLOTS < count ? (b + 1) * HTM_KNN_SLOTS : count; }
// block rows of the distance launch over nq queries
CLS_HD static inline int knn_query_groups(int nq, int queries) { return (nq + queries - 1) / queries; }
// the largest overlap two patterns can have, and the select's bins: an overlap's bin is overlap >> shift, the smallest shift that
// leaves fewer than HTM_KNN_BINS bins; its place inside the bin is overlap & ((1 << shift) - 1)
CLS_HD static inline int knn_max_overlap(int max_pairs, int K) { return max_pairs * (K < 32 ? K : 32); }
CLS_HD static inline int knn_shift(int max_overlap) {
    int s = 0;
    while ((max_overlap >> s) >= HTM_KNN_BINS) ++s;
    return s;
}
CLS_HD static inline int knn_bin(int overlap, int shift) { return overlap >> shift; }
// slots of one wave's share of the select's walk over `count` slots: a quarter, in whole wave rows
CLS_HD static inline int knn_wave_span(int count) { return ((count + 3) / 4 + 63) / 64 * 64; }

#ifdef __HIPCC__

struct KnnDev {
    int32_t labels, k, min_overlap, capacity, K, WPC, n_cols, max_pairs, words, queries, in_lds, shift, bitmap;
    ClsPair *store;             // [capacity][max_pairs]
    int32_t *label;             // [capacity]
    int64_t *stamp;             // [capacity]
    uint16_t *ovl;              // [HTM_KNN_CHUNK][capacity]: the overlaps of the chunk in flight
    uint32_t *table;            // [HTM_KNN_CHUNK][words], zero between chunks (null while the tables fit LDS)
};

// a call's inputs: the call's arrays, the step total before it and the slots in use before and behind its append
struct KnnStep {
    const ClsPair *pairs;       // [n_steps][pairs_per_step]
    int32_t pairs_per_step;
    const int32_t *labels;      // [n_labels]
    int32_t n_labels, first_step, n_steps;
    int32_t *best;              // [n_steps][5]
    int32_t *votes;             // [n_steps][labels] or null
    int64_t total;
    int32_t count0, count;
};

__device__ __forceinline__ int32_t knn_label_of(const KnnDev &d, const KnnStep &s, int i) {
    const int32_t g = s.labels[(int)(((int64_t)s.first_step + i) % s.n_labels)];
    return g >= 0 && g < d.labels ? g : -1;
}

__device__ __forceinline__ uint2 knn_load_pair(const ClsPair *p) { return *(const uint2 *)p; }

// one block: pos[i] = the slot step i of the call stores its pattern in (count0 + the labelled steps before it), -1 for a step
// without a label.  A thread takes a run of steps; the runs' counts are scanned in LDS.
__device__ __forceinline__ void knn_place_block(const KnnDev &d, const KnnStep &s, int32_t *__restrict__ pos) {
    __shared__ int s_scan[256];
    const int tid = (int)threadIdx.x, run = (s.n_steps + 255) / 256;
    const int lo = min(tid * run, s.n_steps), hi = min(lo + run, s.n_steps);
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += knn_label_of(d, s, i) >= 0;
    s_scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int at = s.count0 + s_scan[tid] - mine;
    for (int i = lo; i < hi; ++i) pos[i] = knn_label_of(d, s, i) >= 0 ? at++ : -1;
}

__global__ __launch_bounds__(256) void kknn_place(KnnDev d, KnnStep s, int32_t *__restrict__ pos) { knn_place_block(d, s, pos); }

// pair e of the call's steps: a labelled step's row into its slot (padded with (-1, 0)), label and stamp with pair 0
__device__ __forceinline__ void knn_append_pair(const KnnDev &d, const KnnStep &s, const int32_t *__restrict__ pos, int64_t e) {
    const int i = (int)(e / d.max_pairs), j = (int)(e % d.max_pairs);
    if (i >= s.n_steps) return;
    const int slot = pos[i];
    if (slot < 0 || slot >= d.capacity) return;
    uint2 pr = make_uint2(0xFFFFFFFFu, 0u);
    if (j < s.pairs_per_step) pr = knn_load_pair(s.pairs + (size_t)i * s.pairs_per_step + j);
    *(uint2 *)(d.store + (size_t)slot * d.max_pairs + j) = pr;
    if (j == 0) {
        d.label[slot] = knn_label_of(d, s, i);
        d.stamp[slot] = s.total + i;
    }
}

// a thread per pair of the call's steps
__global__ __launch_bounds__(256) void kknn_append(KnnDev d, KnnStep s, const int32_t *__restrict__ pos) {
    knn_append_pair(d, s, pos, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// pair e of the chunk's queries [first, first + nq): the live bits into the query's row of the global table (fill), or the same
// word zeroed again (fill == 0)
__device__ __forceinline__ void knn_scatter_pair(const KnnDev &d, const KnnStep &s, int first, int nq, int fill, int64_t e) {
    const int q = (int)(e / s.pairs_per_step), j = (int)(e % s.pairs_per_step);
    if (q >= nq) return;
    const uint2 pr = knn_load_pair(s.pairs + (size_t)(first + q) * s.pairs_per_step + j);
    const uint32_t bits = cls_live_bits((int32_t)pr.x, pr.y, d.K, d.WPC, d.n_cols);
    if (!bits) return;
    uint32_t *w = d.table + (size_t)q * d.words + (int32_t)pr.x;
    if (fill) atomicOr(w, bits); else *w = 0u;
}

// a thread per pair of the chunk's queries
__global__ __launch_bounds__(256) void kknn_scatter(KnnDev d, KnnStep s, int first, int nq, int fill) {
    knn_scatter_pair(d, s, first, nq, fill, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// Block (bx, by) of the distance launch over the queries [first, first + nq) and the slots [0, s.count): the overlaps of the queries
// of group by with the slots of block bx (the one-stream kernels: the block's own x and y; a bank's: inside its member).  TABLE_IN_LDS: the group's tables are staged in `lds` (dynamic: queries * words words);
// otherwise they are rows of d.table, filled by kknn_scatter, and `lds` holds the group's presence bitmaps (d.bitmap: queries *
// knn_bitmap_words words; a pair whose bit is not set adds nothing and reads nothing).
template <bool TABLE_IN_LDS>
__device__ __forceinline__ void knn_distance_block(const KnnDev &d, const KnnStep &s, int first, int nq, uint32_t *lds, int bx, int by) {
    __shared__ int s_ov[HTM_KNN_QUERIES * HTM_KNN_SLOTS];
    const int tid = (int)threadIdx.x;
    const int q0 = by * d.queries, nqb = min(d.queries, nq - q0);
    const int slot0 = knn_block_first(bx), ns = knn_block_last(bx, s.count) - slot0;
    for (int e = tid; e < nqb * HTM_KNN_SLOTS; e += 256) s_ov[e] = 0;
    const uint32_t *tab;
    if (TABLE_IN_LDS) {
        for (int e = tid; e < nqb * d.words; e += 256) lds[e] = 0u;
        __syncthreads();
        for (int e = tid; e < nqb * s.pairs_per_step; e += 256) {
            const int q = e / s.pairs_per_step, j = e % s.pairs_per_step;
            const uint2 pr = knn_load_pair(s.pairs + (size_t)(first + q0 + q) * s.pairs_per_step + j);
            const uint32_t bits = cls_live_bits((int32_t)pr.x, pr.y, d.K, d.WPC, d.n_cols);
            if (bits) atomicOr(&lds[q * d.words + (int32_t)pr.x], bits);
        }
        tab = lds;
    } else {
        tab = d.table + (size_t)q0 * d.words;
        if (d.bitmap) {
            const int bw = (int)knn_bitmap_words(d.words);
            for (int e = tid; e < nqb * bw; e += 256) lds[e] = 0u;
            __syncthreads();
            for (int e = tid; e < nqb * s.pairs_per_step; e += 256) {
                const int q = e / s.pairs_per_step, j = e % s.pairs_per_step;
                const uint2 pr = knn_load_pair(s.pairs + (size_t)(first + q0 + q) * s.pairs_per_step + j);
                if (cls_live_bits((int32_t)pr.x, pr.y, d.K, d.WPC, d.n_cols)) atomicOr(&lds[q * bw + ((int32_t)pr.x >> 5)], 1u << (pr.x & 31u));
            }
        }
    }
    __syncthreads();
    // the block's rows are one contiguous run of ns * max_pairs pairs: pair e belongs to slot e / max_pairs, kept without a division
    const ClsPair *rows = d.store + (size_t)slot0 * d.max_pairs;
    const int n_pairs = ns * d.max_pairs, step_slots = 256 / d.max_pairs, step_rest = 256 % d.max_pairs;
    int sl = tid / d.max_pairs, rest = tid % d.max_pairs;
    for (int e = tid; e < n_pairs; e += 256) {
        const uint2 pr = knn_load_pair(rows + e);
        const uint32_t bits = cls_live_bits((int32_t)pr.x, pr.y, d.K, d.WPC, d.n_cols);
        if (bits) {
            const uint32_t *t = tab + (int32_t)pr.x;
            const int bw = (int)knn_bitmap_words(d.words), at = (int32_t)pr.x >> 5;
            for (int q = 0; q < nqb; ++q) {
                if (!TABLE_IN_LDS && d.bitmap && !((lds[q * bw + at] >> (pr.x & 31u)) & 1u)) continue;
                const int ov = knn_pair_overlap(bits, t[(size_t)q * d.words]);
                if (ov) atomicAdd(&s_ov[q * HTM_KNN_SLOTS + sl], ov);
            }
        }
        sl += step_slots;
        rest += step_rest;
        if (rest >= d.max_pairs) { rest -= d.max_pairs; ++sl; }
    }
    __syncthreads();
    for (int e = tid; e < nqb * ns; e += 256) {
        const int q = e / ns, l = e % ns, slot = slot0 + l;
        const bool seen = d.stamp[slot] < s.total + first + q0 + q;
        d.ovl[(size_t)(q0 + q) * d.capacity + slot] = (uint16_t)(seen ? s_ov[q * HTM_KNN_SLOTS + l] : 0);
    }
}

// grid (knn_slot_blocks(count), knn_query_groups(nq, queries)), dynamic LDS knn_distance_lds(words) bytes
__global__ __launch_bounds__(256) void kknn_distance_lds(KnnDev d, KnnStep s, int first, int nq) {
    extern __shared__ uint32_t knn_tables[];
    knn_distance_block<true>(d, s, first, nq, knn_tables, (int)blockIdx.x, (int)blockIdx.y);
}

// the same grid, between kknn_scatter(fill) and kknn_scatter(clear) of the chunk
__global__ __launch_bounds__(256) void kknn_distance_global(KnnDev d, KnnStep s, int first, int nq) {
    extern __shared__ uint32_t knn_tables[];
    knn_distance_block<false>(d, s, first, nq, knn_tables, (int)blockIdx.x, (int)blockIdx.y);
}

// the largest of v over the block (every thread calls it; s_red: 4 words of 64 bits)
__device__ __forceinline__ unsigned long long knn_block_max(unsigned long long v, unsigned long long *s_red) {
    for (int off = 32; off; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    __syncthreads();                                        // (s_red is free again)
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = s_red[0];
    for (int w = 1; w < 4; ++w) v = s_red[w] > v ? s_red[w] : v;
    return v;
}

// one block selects for query first + q over the overlaps d.ovl[q][0 .. count)
__device__ __forceinline__ void knn_select_block(const KnnDev &d, const KnnStep &s, int first, int q) {
    __shared__ int s_hist[HTM_KNN_BINS];
    __shared__ int s_votes[HTM_KNN_MAX_LABELS];
    __shared__ int s_scan[256];
    __shared__ int s_pick[2];                               // the bin (then the value) of the k-th overlap, the candidates above it
    __shared__ int s_wave[4];
    __shared__ unsigned long long s_red[4];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = first + q, count = s.count;
    const uint16_t *__restrict__ row = d.ovl + (size_t)q * d.capacity;
    for (int b = tid; b < HTM_KNN_BINS; b += 256) s_hist[b] = 0;
    for (int l = tid; l < d.labels; l += 256) s_votes[l] = 0;
    __syncthreads();
    for (int slot = tid; slot < count; slot += 256) {
        const int key = row[slot];
        if (key >= d.min_overlap) atomicAdd(&s_hist[knn_bin(key, d.shift)], 1);
    }
    __syncthreads();
    // the candidates in this thread's eight bins and in all bins above them
    int mine = 0;
    for (int b = 0; b < HTM_KNN_BINS / 256; ++b) mine += s_hist[tid * (HTM_KNN_BINS / 256) + b];
    s_scan[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid + off < 256 ? s_scan[tid + off] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    const int n_cand = s_scan[0];
    // v: every candidate above v is a neighbour, and the `ties` lowest slots at v (fewer than k candidates: all of them, v = 0)
    int v = 0, ties = 0;
    if (n_cand > d.k) {                                     // (block-uniform)
        const int above_me = tid < 255 ? s_scan[tid + 1] : 0;
        if (s_scan[tid] >= d.k && above_me < d.k) {         // (one thread: the k-th overlap is in its bins)
            int cum = above_me;
            for (int b = HTM_KNN_BINS / 256 - 1; b >= 0; --b) {
                const int n = s_hist[tid * (HTM_KNN_BINS / 256) + b];
                if (cum + n >= d.k) { s_pick[0] = tid * (HTM_KNN_BINS / 256) + b; s_pick[1] = cum; break; }
                cum += n;
            }
        }
        __syncthreads();
        int pick = s_pick[0], above = s_pick[1];
        if (d.shift > 0) {                                  // the overlaps inside the bin, at most 32 of them
            __syncthreads();
            if (tid < (1 << d.shift)) s_hist[tid] = 0;
            __syncthreads();
            for (int slot = tid; slot < count; slot += 256) {
                const int key = row[slot];
                if (key >= d.min_overlap && knn_bin(key, d.shift) == pick) atomicAdd(&s_hist[key & ((1 << d.shift) - 1)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int cum = above;
                for (int low = (1 << d.shift) - 1; low >= 0; --low) {
                    if (cum + s_hist[low] >= d.k) { s_pick[0] = (pick << d.shift) | low; s_pick[1] = cum; break; }
                    cum += s_hist[low];
                }
            }
            __syncthreads();
            pick = s_pick[0];
            above = s_pick[1];
        }
        v = pick;
        ties = d.k - above;
    }
    // the walk in slot order, a wave per quarter of the slots: first the ties in each quarter, then the neighbours
    const int span = knn_wave_span(count), lo = min(wave * span, count), hi = min(lo + span, count);
    int before = 0;
    if (ties > 0) {
        int n = 0;
        for (int base = lo; base < hi; base += 64)
            n += __popcll(__ballot(base + lane < hi && row[base + lane] == v));
        if (lane == 0) s_wave[wave] = n;
        __syncthreads();
        for (int w = 0; w < wave; ++w) before += s_wave[w];
    }
    unsigned long long best = 0ull;
    for (int base = lo; base < hi; base += 64) {
        const int slot = base + lane;
        const int key = slot < hi ? row[slot] : 0;
        const bool tie = ties > 0 && key == v && slot < hi;
        const unsigned long long tied = __ballot(tie);
        const int rank = before + __popcll(tied & ((1ull << lane) - 1ull));
        before += __popcll(tied);
        if ((key > v && key >= d.min_overlap) || (tie && rank < ties)) {
            const int32_t l = d.label[slot];
            if (l >= 0 && l < d.labels) atomicAdd(&s_votes[l], 1);
            const unsigned long long mark = ((unsigned long long)key << 32) | (0xFFFFFFFFu - (uint32_t)slot);
            best = mark > best ? mark : best;
        }
    }
    best = knn_block_max(best, s_red);                      // (its barriers: the votes are all in)
    unsigned long long top = 0ull;
    for (int l = tid; l < d.labels; l += 256) {
        const unsigned long long mark = ((unsigned long long)s_votes[l] << 32) | (0xFFFFFFFFu - (uint32_t)l);
        top = mark > top ? mark : top;
    }
    top = knn_block_max(top, s_red);
    if (tid == 0) {
        int32_t *o = s.best + (size_t)i * 5;
        if (best) {
            const int slot = (int)(0xFFFFFFFFu - (uint32_t)best);
            o[0] = (int32_t)(0xFFFFFFFFu - (uint32_t)top);
            o[1] = (int32_t)(top >> 32);
            o[2] = (int32_t)(best >> 32);
            o[3] = slot;
            o[4] = (int32_t)(uint32_t)d.stamp[slot];
        } else {
            o[0] = -1; o[1] = 0; o[2] = 0; o[3] = -1; o[4] = -1;
        }
    }
    if (s.votes) {
        int32_t *o = s.votes + (size_t)i * d.labels;
        for (int l = tid; l < d.labels; l += 256) o[l] = s_votes[l];
    }
}

// grid nq: block q selects for query first + q
__global__ __launch_bounds__(256) void kknn_select(KnnDev d, KnnStep s, int first) { knn_select_block(d, s, first, (int)blockIdx.x); }

#endif  // __HIPCC__
#endif
