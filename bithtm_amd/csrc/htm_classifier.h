// SDR classifier on the device (htm_classifier_*, include/bithtm_hip.h; the definition is
// bithtm_amd/classifier.py, which this file equals bit for bit).  One object keeps, per horizon h, the weight table
// W[h][unit][B_pad] (int32 in units of 2^-16, rows contiguous, B_pad = buckets rounded up to 4 so that a lane loads 16 bytes),
// the ring of the last max(steps) + 1 patterns (max_pairs (index, word) pairs each, unused pairs (-1, 0)) and the count of
// patterns since the history was last emptied.  The total step count, which names the ring slots, is the host's.
//
// A learning step is two launches:
//   kcls_sum    grid (blocks, H): the blocks split the pairs of P_t (the call's row) and of P_(t-h) (the ring's); a wave takes a pair,
//               its lanes four buckets each of every row the pair's word names; per-bucket sums in registers, then in LDS, then one
//               64-bit integer atomic per bucket and block into the horizon's accumulator (integer sums: any split is exact).  The
//               block that draws the last ticket of its horizon -- behind an agent-scope release fence; it acquires before it reads
//               -- takes both softmaxes in LDS, writes the step's outputs and delta[h][B_pad], and leaves accumulator and ticket zero.
//               The blocks of horizon 0 copy P_t into the ring (the slot of step t - ring_len, which no horizon reads).
//   kcls_apply  grid (blocks, H): W[h][u][b] = clamp(W[h][u][b] + delta[h][b]) over the units of P_(t-h), read from the ring; returns
//               at once where kcls_sum found nothing to learn.  Block (0, 0) advances the count (kcls_sum's blocks have all read it).
// A frozen call (learn == 0) has no dependence between its steps: kcls_frozen is kcls_sum's P_t half, up to
// HTM_CLASSIFIER_CHUNK steps per launch (step and horizon share grid y) over accumulators sized for the chunk.  No block ever waits for another.
// kcls_capture fills a recorded run's pattern rows (htm_set_run_active_cells).
// Each of the four is written once, as a device function over the ClsDev and ClsStep of one stream (cls_sum_block, cls_apply_block,
// cls_frozen_block, cls_capture_rows); the kcls_ kernels call it for the object's one stream, the kgcls_ kernels of a bank (below) for
// the stream of the block's row.
// The arithmetic is in the __host__ __device__ functions at the top: tests/host_stub/classifier_host.cpp evaluates them on the host.
// Part of the single translation unit htm_engine.hip (included after htm_likelihood.h).
#ifndef BITHTM_HTM_CLASSIFIER_H
#define BITHTM_HTM_CLASSIFIER_H

#include <stdint.h>

#ifdef __HIPCC__
#define CLS_HD __host__ __device__
#else
#define CLS_HD
#endif

#define HTM_CLASSIFIER_CHUNK 512            // steps per frozen launch (bithtm_amd/_lib.py: CLASSIFIER_CHUNK)
#define HTM_CLASSIFIER_THREADS 256          // four waves: a wave per pair
#define HTM_CLASSIFIER_PAIRS 16             // pairs of a pattern per block (bithtm_amd/_lib.py: CLASSIFIER_PAIRS)
#define HTM_CLASSIFIER_MAX_BUCKETS 1024
#define HTM_CLASSIFIER_MAX_HORIZONS 8
#define HTM_CLASSIFIER_MAX_HORIZON 64
#define HTM_CLASSIFIER_EXP 2049             // entries of the table: T[i] = round(2^30 * exp(-i / 64))
#define HTM_CLASSIFIER_W_LIMIT (1 << 30)

// 2^30 * exp(-d / 65536) for d >= 0 by linear interpolation in the table; 0 from 32.0 on
CLS_HD static inline int32_t cls_exp(int64_t d, const int32_t *T) {
    if (d >= ((int64_t)32 << 16)) return 0;
    const int i = (int)(d >> 10);
    const int64_t f = d & 1023;
    const int64_t t0 = T[i];
    return (int32_t)(t0 - (((t0 - (int64_t)T[i + 1]) * f) >> 10));
}

// p of a bucket in units of 2^-16 from its e and the sum of all of them (z >= 2^30: the largest activation's e)
CLS_HD static inline int32_t cls_prob(int32_t e, int64_t z) { return (int32_t)((uint64_t)((int64_t)e << 16) / (uint64_t)z); }

// the weight step of a bucket: alpha_q * (onehot - p) / 65536, truncated toward zero
CLS_HD static inline int32_t cls_delta(int32_t alpha_q, int32_t p, int is_target) {
    const int64_t x = (int64_t)alpha_q * ((is_target ? 65536 : 0) - p);
    return x < 0 ? -(int32_t)((-x) >> 16) : (int32_t)(x >> 16);
}

CLS_HD static inline int32_t cls_clamp(int32_t w, int32_t d) {
    const int64_t v = (int64_t)w + d;
    return (int32_t)(v > HTM_CLASSIFIER_W_LIMIT ? HTM_CLASSIFIER_W_LIMIT : v < -HTM_CLASSIFIER_W_LIMIT ? -HTM_CLASSIFIER_W_LIMIT : v);
}

// the bits of word `index` of a pattern that are cells of a column below n_cols (cell_dim K, WPC words per column): 0 for an index
// outside the table -- nothing a pattern holds makes a kernel read or write outside the weights
CLS_HD static inline uint32_t cls_live_bits(int32_t index, uint32_t word, int K, int WPC, int n_cols) {
    if (index < 0 || index / WPC >= n_cols) return 0u;
    const int top = K - (index % WPC) * 32;
    return top >= 32 ? word : (word & ((1u << top) - 1u));
}

// first unit of word `index` (a live one)
CLS_HD static inline int64_t cls_unit0(int32_t index, int K, int WPC) { return (int64_t)(index / WPC) * K + (int64_t)(index % WPC) * 32; }

#ifdef __HIPCC__

struct ClsPair { int32_t index; uint32_t word; };

struct ClsDev {
    int32_t B, B_pad, H, K, WPC, n_cols, alpha_q, max_pairs, ring_len;
    int32_t steps[HTM_CLASSIFIER_MAX_HORIZONS];
    int32_t *w;                 // [H][units][B_pad]
    int64_t w_stride;           // units * B_pad
    ClsPair *ring;              // [ring_len][max_pairs]
    int64_t *count;             // patterns since the history was last emptied
    int64_t *acc;               // [H][2][B_pad]: the sums over P_t and P_(t-h) of the step in flight, zero between launches
    uint32_t *ticket;           // [H] blocks arrived, zero between launches
    int32_t *delta;             // [H][B_pad]
    int32_t *learn;             // [H] 1: kcls_apply has this horizon's delta to add
    const int32_t *exp_table;   // [2049]
};

// the frozen call's accumulators: [chunk][H][B_pad] sums and [chunk][H] tickets, zero between launches
struct ClsFrozen { int64_t *acc; uint32_t *ticket; };

// one step's inputs as its launches take them: the call's arrays, the step's index in the call and its absolute index
struct ClsStep {
    const ClsPair *pairs;       // [n_steps][pairs_per_step]
    int32_t pairs_per_step;
    const int32_t *targets;     // [n_targets]
    const uint32_t *reset_bits; // [ceil(n_targets / 32)] or null
    int32_t n_targets, first_step;
    int32_t *best;              // [n_steps][H][2]
    int32_t *dist;              // [n_steps][H][B] or null
    int64_t total;              // steps the object had seen before this call
};

__device__ __forceinline__ int cls_reset_bit(const ClsStep &s, int i) {
    if (!s.reset_bits) return 0;
    const uint32_t row = (uint32_t)(((int64_t)s.first_step + i) % s.n_targets);
    return (int)((s.reset_bits[row >> 5] >> (row & 31)) & 1u);
}

// The block's share of a pattern's rows summed per bucket into s_acc[B_pad] (LDS, int64, zeroed by the caller before a barrier):
// pairs [lo, hi) of `pairs`, a wave per pair, a lane per four buckets.  Every row read lies inside W[h]: cls_live_bits.
__device__ __forceinline__ void cls_sum_rows(const ClsDev &c, const int32_t *__restrict__ wh, const ClsPair *__restrict__ pairs, int lo, int hi,
                                             unsigned long long *s_acc) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    for (int b0 = 0; b0 < c.B_pad; b0 += 256) {
        const int b = b0 + 4 * lane;
        if (b >= c.B_pad) continue;
        int64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (int j = lo + wave; j < hi; j += HTM_CLASSIFIER_THREADS / 64) {
            const ClsPair pr = pairs[j];
            uint32_t bits = cls_live_bits(pr.index, pr.word, c.K, c.WPC, c.n_cols);
            if (!bits) continue;
            const int32_t *row0 = wh + cls_unit0(pr.index, c.K, c.WPC) * c.B_pad + b;
            while (bits) {
                const int bit = __ffs(bits) - 1;
                bits &= bits - 1;
                const int4 v = *(const int4 *)(row0 + (int64_t)bit * c.B_pad);
                a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
            }
        }
        if (a0) atomicAdd(&s_acc[b], (unsigned long long)a0);
        if (a1) atomicAdd(&s_acc[b + 1], (unsigned long long)a1);
        if (a2) atomicAdd(&s_acc[b + 2], (unsigned long long)a2);
        if (a3) atomicAdd(&s_acc[b + 3], (unsigned long long)a3);
    }
}

// The block's LDS sums into the global accumulator, then the ticket: returns (to every thread) whether this block is the last of
// `blocks` to arrive.  The order is the last-block reducer's: every wave's atomics drained, the block's barrier, one lane's
// agent-scope release, its wait, then the relaxed agent-scope ticket add; the last block acquires before anyone reads.
__device__ __forceinline__ bool cls_arrive(unsigned long long *acc, const unsigned long long *s_acc, int n, uint32_t *ticket, uint32_t blocks,
                                           uint32_t *s_last) {
    for (int b = (int)threadIdx.x; b < n; b += HTM_CLASSIFIER_THREADS)
        if (s_acc[b]) __hip_atomic_fetch_add(&acc[b], s_acc[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t last = drawn == blocks - 1u;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *s_last = last;
    }
    __syncthreads();
    return *s_last != 0u;
}

// The last block: the accumulator's n sums into LDS (agent-scope loads: they were made by other blocks' atomics) and zero behind them
__device__ __forceinline__ void cls_take(unsigned long long *acc, unsigned long long *s_acc, int n) {
    for (int b = (int)threadIdx.x; b < n; b += HTM_CLASSIFIER_THREADS) {
        s_acc[b] = __hip_atomic_load(&acc[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&acc[b], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
}

// Softmax over a[0 .. B) (LDS, int64) by the whole block: e into s_e[B], -> the lowest bucket with the largest a, and the sum of e.
// s_red: 2 * 4 + 1 words of 64 bits.  Every thread calls it (barriers).
__device__ __forceinline__ void cls_softmax(const ClsDev &c, const unsigned long long *s_acc, int32_t *s_e, unsigned long long *s_red, int &best, int64_t &z) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // the largest activation and its lowest bucket: per thread, per wave, per block
    int64_t m = INT64_MIN;
    int mb = 0x7fffffff;
    for (int b = tid; b < c.B; b += HTM_CLASSIFIER_THREADS) {
        const int64_t a = (int64_t)s_acc[b];
        if (a > m) { m = a; mb = b; }                     // (ascending b: the first of equals stays)
    }
    for (int off = 32; off; off >>= 1) {
        const int64_t om = __shfl_xor(m, off);
        const int ob = __shfl_xor(mb, off);
        if (om > m || (om == m && ob < mb)) { m = om; mb = ob; }
    }
    if (lane == 0) { s_red[wave] = (unsigned long long)m; s_red[4 + wave] = (unsigned long long)(uint32_t)mb; }
    __syncthreads();
    m = (int64_t)s_red[0];
    mb = (int)s_red[4];
    for (int w = 1; w < HTM_CLASSIFIER_THREADS / 64; ++w) {
        const int64_t om = (int64_t)s_red[w];
        const int ob = (int)s_red[4 + w];
        if (om > m || (om == m && ob < mb)) { m = om; mb = ob; }
    }
    if (tid == 0) s_red[8] = 0ull;
    __syncthreads();
    int64_t sum = 0;
    for (int b = tid; b < c.B; b += HTM_CLASSIFIER_THREADS) {
        const int32_t e = cls_exp(m - (int64_t)s_acc[b], c.exp_table);
        s_e[b] = e;
        sum += e;
    }
    for (int off = 32; off; off >>= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) atomicAdd(&s_red[8], (unsigned long long)sum);
    __syncthreads();
    best = mb;
    z = (int64_t)s_red[8];
    __syncthreads();                                       // (s_red is free again)
}

// the step's outputs of horizon h from the softmax of P_t
__device__ __forceinline__ void cls_write_outputs(const ClsDev &c, const ClsStep &s, int i, int h, const int32_t *s_e, int best, int64_t z) {
    if (threadIdx.x == 0) {
        int32_t *o = s.best + ((size_t)i * c.H + h) * 2;
        o[0] = best;
        o[1] = cls_prob(s_e[best], z);
    }
    if (s.dist) {
        int32_t *o = s.dist + ((size_t)i * c.H + h) * (size_t)c.B;
        for (int b = (int)threadIdx.x; b < c.B; b += HTM_CLASSIFIER_THREADS) o[b] = cls_prob(s_e[b], z);
    }
}

// P_t (the pairs [lo, hi) of it that exist, then (-1, 0)) into ring slot `slot`
__device__ __forceinline__ void cls_ring_copy(const ClsDev &c, const ClsPair *__restrict__ row, int n_pairs, int lo, int hi, int slot) {
    ClsPair *dst = c.ring + (size_t)slot * c.max_pairs;
    for (int j = lo + (int)threadIdx.x; j < hi; j += HTM_CLASSIFIER_THREADS) dst[j] = j < n_pairs ? row[j] : ClsPair{-1, 0u};
}

// Step i of a learning call, horizon index h (its `horizon` = steps[h], read by the kernel from its own argument), the block's share:
// the body of kcls_sum and kgcls_sum, over the ClsDev and ClsStep of the block's stream.  Grid x = ceil(max_pairs / HTM_CLASSIFIER_PAIRS).
__device__ __forceinline__ void cls_sum_block(const ClsDev &c, const ClsStep &s, int h, int horizon, int i) {
    __shared__ unsigned long long s_acc[2 * HTM_CLASSIFIER_MAX_BUCKETS];
    __shared__ int32_t s_e[HTM_CLASSIFIER_MAX_BUCKETS];
    __shared__ unsigned long long s_red[9];
    __shared__ uint32_t s_last;
    const int tid = (int)threadIdx.x;
    const int64_t t = s.total + i;
    const int64_t count = cls_reset_bit(s, i) ? 0 : *c.count;               // patterns of the stream's history before P_t enters
    const int32_t g = s.targets[(int)(((int64_t)s.first_step + i) % s.n_targets)];
    const bool learns = g >= 0 && g < c.B && (int64_t)horizon <= count;    // (the history then holds P_(t-h); block-uniform)
    const int lo = (int)blockIdx.x * HTM_CLASSIFIER_PAIRS, hi = min(lo + HTM_CLASSIFIER_PAIRS, c.max_pairs);
    const ClsPair *row = s.pairs + (size_t)i * s.pairs_per_step;
    const int32_t *wh = c.w + (int64_t)h * c.w_stride;
    for (int b = tid; b < 2 * c.B_pad; b += HTM_CLASSIFIER_THREADS) s_acc[b] = 0ull;
    __syncthreads();
    cls_sum_rows(c, wh, row, min(lo, s.pairs_per_step), min(hi, s.pairs_per_step), s_acc);
    if (learns) {
        if (horizon == 0) cls_sum_rows(c, wh, row, min(lo, s.pairs_per_step), min(hi, s.pairs_per_step), s_acc + c.B_pad);
        else cls_sum_rows(c, wh, c.ring + (size_t)((t - horizon) % c.ring_len) * c.max_pairs, lo, hi, s_acc + c.B_pad);
    }
    if (h == 0) cls_ring_copy(c, row, s.pairs_per_step, lo, hi, (int)(t % c.ring_len));
    __syncthreads();
    unsigned long long *acc = (unsigned long long *)c.acc + (size_t)h * 2 * c.B_pad;
    if (!cls_arrive(acc, s_acc, 2 * c.B_pad, c.ticket + h, gridDim.x, &s_last)) return;
    cls_take(acc, s_acc, 2 * c.B_pad);
    if (tid == 0) {
        __hip_atomic_store(c.ticket + h, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c.learn[h] = learns ? 1 : 0;
    }
    int best;
    int64_t z;
    cls_softmax(c, s_acc, s_e, s_red, best, z);
    cls_write_outputs(c, s, i, h, s_e, best, z);
    if (!learns) return;                                   // (block-uniform)
    __syncthreads();                                       // (s_e is read above, written below)
    cls_softmax(c, s_acc + c.B_pad, s_e, s_red, best, z);
    int32_t *delta = c.delta + (size_t)h * c.B_pad;
    for (int b = tid; b < c.B_pad; b += HTM_CLASSIFIER_THREADS) delta[b] = b < c.B ? cls_delta(c.alpha_q, cls_prob(s_e[b], z), b == g) : 0;
}

// Behind cls_sum_block of the same step, on the same grid: the body of kcls_apply and kgcls_apply
__device__ __forceinline__ void cls_apply_block(const ClsDev &c, const ClsStep &s, int h, int horizon, int i) {
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    if (blockIdx.x == 0 && h == 0 && threadIdx.x == 0) *c.count = (cls_reset_bit(s, i) ? 0 : *c.count) + 1;
    if (!c.learn[h]) return;
    const int64_t t = s.total + i;
    const ClsPair *pairs = c.ring + (size_t)((t - horizon) % c.ring_len) * c.max_pairs;
    const int lo = (int)blockIdx.x * HTM_CLASSIFIER_PAIRS, hi = min(lo + HTM_CLASSIFIER_PAIRS, c.max_pairs);
    int32_t *wh = c.w + (int64_t)h * c.w_stride;
    const int32_t *delta = c.delta + (size_t)h * c.B_pad;
    for (int b0 = 0; b0 < c.B_pad; b0 += 256) {
        const int b = b0 + 4 * lane;
        if (b >= c.B_pad) continue;
        const int4 d = *(const int4 *)(delta + b);
        for (int j = lo + wave; j < hi; j += HTM_CLASSIFIER_THREADS / 64) {
            const ClsPair pr = pairs[j];
            uint32_t bits = cls_live_bits(pr.index, pr.word, c.K, c.WPC, c.n_cols);
            if (!bits) continue;
            int32_t *row0 = wh + cls_unit0(pr.index, c.K, c.WPC) * c.B_pad + b;
            while (bits) {
                const int bit = __ffs(bits) - 1;
                bits &= bits - 1;
                int4 *p = (int4 *)(row0 + (int64_t)bit * c.B_pad);
                int4 v = *p;
                v.x = cls_clamp(v.x, d.x); v.y = cls_clamp(v.y, d.y); v.z = cls_clamp(v.z, d.z); v.w = cls_clamp(v.w, d.w);
                *p = v;
            }
        }
    }
}

// Step first + zi of the n steps [first, first + n) of a frozen launch, horizon index h, the block's share: the body of kcls_frozen and
// kgcls_frozen.  A block row's row of the accumulators f is its own: blockIdx.y.  Grid x = ceil(pairs_per_step / HTM_CLASSIFIER_PAIRS).
__device__ __forceinline__ void cls_frozen_block(const ClsDev &c, const ClsFrozen &f, const ClsStep &s, int h, int zi, int first, int n) {
    __shared__ unsigned long long s_acc[HTM_CLASSIFIER_MAX_BUCKETS];
    __shared__ int32_t s_e[HTM_CLASSIFIER_MAX_BUCKETS];
    __shared__ unsigned long long s_red[9];
    __shared__ uint32_t s_last;
    __shared__ int s_reset;
    const int i = first + zi, tid = (int)threadIdx.x;
    const int64_t t = s.total + i;
    const int lo = (int)blockIdx.x * HTM_CLASSIFIER_PAIRS, hi = min(lo + HTM_CLASSIFIER_PAIRS, s.pairs_per_step);
    const ClsPair *row = s.pairs + (size_t)i * s.pairs_per_step;
    // the stream's count behind the chunk: the steps since its last reset, or n more (one block; nobody reads the count in this launch)
    if (blockIdx.x == 0 && h == 0 && zi == 0) {
        if (tid == 0) s_reset = -1;
        __syncthreads();
        for (int j = tid; j < n; j += HTM_CLASSIFIER_THREADS)
            if (cls_reset_bit(s, first + j)) atomicMax(&s_reset, j);
        __syncthreads();
        if (tid == 0) *c.count = s_reset < 0 ? *c.count + n : (int64_t)(n - s_reset);
    }
    // the stream's ring takes the chunk's last ring_len patterns (distinct slots), the whole row of each
    if (h == 0 && zi >= n - c.ring_len)
        for (int l = lo; l < c.max_pairs; l += (int)gridDim.x * HTM_CLASSIFIER_PAIRS)
            cls_ring_copy(c, row, s.pairs_per_step, l, min(l + HTM_CLASSIFIER_PAIRS, c.max_pairs), (int)(t % c.ring_len));
    for (int b = tid; b < c.B_pad; b += HTM_CLASSIFIER_THREADS) s_acc[b] = 0ull;
    __syncthreads();
    cls_sum_rows(c, c.w + (int64_t)h * c.w_stride, row, lo, hi, s_acc);
    __syncthreads();
    unsigned long long *acc = (unsigned long long *)f.acc + (size_t)blockIdx.y * c.B_pad;
    uint32_t *ticket = f.ticket + blockIdx.y;
    if (!cls_arrive(acc, s_acc, c.B_pad, ticket, gridDim.x, &s_last)) return;
    cls_take(acc, s_acc, c.B_pad);
    if (tid == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int best;
    int64_t z;
    cls_softmax(c, s_acc, s_e, s_red, best, z);
    cls_write_outputs(c, s, i, h, s_e, best, z);
}

// grid (ceil(max_pairs / HTM_CLASSIFIER_PAIRS), H): step i of a learning call
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kcls_sum(ClsDev c, ClsStep s, int i) {
    cls_sum_block(c, s, (int)blockIdx.y, c.steps[blockIdx.y], i);
}

// the same grid, behind kcls_sum of the same step
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kcls_apply(ClsDev c, ClsStep s, int i) {
    cls_apply_block(c, s, (int)blockIdx.y, c.steps[blockIdx.y], i);
}

// grid (ceil(pairs_per_step / HTM_CLASSIFIER_PAIRS), H * n), n <= HTM_CLASSIFIER_CHUNK: steps [first, first + n) of a frozen call, block row y
// being horizon y % H of step first + y / H; the accumulators f hold HTM_CLASSIFIER_CHUNK * H rows
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kcls_frozen(ClsDev c, ClsFrozen f, ClsStep s, int first, int n) {
    cls_frozen_block(c, f, s, (int)blockIdx.y % c.H, (int)blockIdx.y / c.H, first, n);
}

// Pattern capture of a recorded htm_run (htm_set_run_active_cells): the device descriptor of the caller's rows (one per handle; graphs
// hold its address, the setter fills it)
struct ClsCapDev { ClsPair *rows; };       // [n][k * WPC]

// Directly behind the record launch of the step of parity p (htm_record.h: every buffer of step t still holds there in every
// schedule): row `slot` of the call takes the k * WPC active-cell words of the step's active columns, in active_cols order.  The slot
// is the record's; a step outside the call's records writes nothing.  A thread per pair: grid x >= k * WPC / 256 blocks.  The body of
// kcls_capture and kgcls_capture, over the Dev, the record descriptor and the capture descriptor of the block's model.
__device__ __forceinline__ void cls_capture_rows(const Dev &d, int p, const RecDev *r, const ClsCapDev &cap) {
    const uint32_t slot = d.ctr->step[p] - r->base;
    if (slot >= (uint32_t)r->n) return;
    const int per = d.k * d.WPC, i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= per) return;
    const int col = d.active_cols[p][i / d.WPC];
    ClsPair pr{-1, 0u};
    if (col >= 0 && col < d.C) {
        pr.index = col * d.WPC + i % d.WPC;
        pr.word = d.act[p][pr.index];
    }
    cap.rows[(size_t)slot * per + i] = pr;
}

__global__ __launch_bounds__(256) void kcls_capture(Dev d, int p, const RecDev *r, const ClsCapDev *cap) { cls_capture_rows(d, p, r, *cap); }

#endif  // __HIPCC__

// ------------------------------------------------------------------------------------------
// A bank of classifiers (htm_classifiers_*): n independent streams of one config, member-major -- weights
// [n][H][units][B_pad] (or one table every member reads: member stride 0), rings [n][ring_len][max_pairs], counts [n], accumulators
// [n][H][2][B_pad], tickets, deltas and learn flags [n][H].  Its kernels run the bodies above (cls_sum_block, cls_apply_block,
// cls_frozen_block, cls_capture_rows): the member shares grid y with the horizon (and, frozen, with the step), a block makes its
// member's ClsDev and ClsStep (gcls_dev, gcls_step) and everything it touches is its member's.  Where a block's row lies is the
// arithmetic below; tests/host_stub/group_classifier_host.cpp evaluates it on the host.

// steps per frozen launch of a bank of n streams: member, step and horizon share grid y (at most 65535 rows)
CLS_HD static inline int gcls_chunk(int n, int H) { const int most = 65535 / (n * H); return most < HTM_CLASSIFIER_CHUNK ? most : HTM_CLASSIFIER_CHUNK; }
// block row y of a learning launch: y = member * H + horizon
CLS_HD static inline int gcls_member(int y, int H) { return y / H; }
CLS_HD static inline int gcls_horizon(int y, int H) { return y % H; }
// block row y of a frozen launch over n steps: y = (member * n + step) * H + horizon
CLS_HD static inline int gcls_frozen_member(int y, int H, int n) { return y / H / n; }
CLS_HD static inline int gcls_frozen_step(int y, int H, int n) { return y / H % n; }
// member m's (horizon h's) row of the [n][H] arrays: tickets and learn flags; times B_pad the deltas, times 2 * B_pad the accumulators
CLS_HD static inline int64_t gcls_row(int m, int H, int h) { return (int64_t)m * H + h; }
// member m's first output row of a call of n_steps steps: best [n][n_steps][H][2], dist [n][n_steps][H][B]
CLS_HD static inline int64_t gcls_out_row(int m, int n_steps, int H) { return (int64_t)m * n_steps * H; }

#ifdef __HIPCC__

struct GClsDev {
    ClsDev c;                   // member 0's
    int32_t n;                  // streams
    int64_t w_member;           // H * w_stride, or 0 where every member reads one table
};

// a call's inputs: per member a device pointer from the call's table, or (no table) member 0's plus a stride per member
struct GClsStep {
    const ClsPair *const *pairs_tab;        // [n] -> [n_steps][pairs_per_step]
    const int32_t *const *targets_tab;      // [n] -> [n_targets]
    const uint32_t *const *resets_tab;      // [n] -> [ceil(n_targets / 32)], or null
    const ClsPair *pairs;
    const int32_t *targets;
    const uint32_t *reset_bits;             // or null
    int64_t pairs_stride, targets_stride, resets_stride;        // in elements
    int32_t pairs_per_step, n_targets, first_step, n_steps;
    int32_t *best;                          // [n][n_steps][H][2]
    int32_t *dist;                          // [n][n_steps][H][B] or null
    int64_t total;
};

// member m's view of the bank: a ClsDev whose pointers are the member's (its steps[] is not to be indexed: read g.c.steps)
__device__ __forceinline__ ClsDev gcls_dev(const GClsDev &g, int m) {
    ClsDev c = g.c;
    c.w += (int64_t)m * g.w_member;
    c.ring += (size_t)m * c.ring_len * c.max_pairs;
    c.count += m;
    c.acc += gcls_row(m, c.H, 0) * 2 * c.B_pad;
    c.ticket += gcls_row(m, c.H, 0);
    c.delta += gcls_row(m, c.H, 0) * c.B_pad;
    c.learn += gcls_row(m, c.H, 0);
    return c;
}

__device__ __forceinline__ ClsStep gcls_step(const GClsStep &g, const ClsDev &c, int m) {
    ClsStep s;
    s.pairs = g.pairs_tab ? g.pairs_tab[m] : g.pairs + (int64_t)m * g.pairs_stride;
    s.targets = g.targets_tab ? g.targets_tab[m] : g.targets + (int64_t)m * g.targets_stride;
    s.reset_bits = g.resets_tab ? g.resets_tab[m] : g.reset_bits ? g.reset_bits + (int64_t)m * g.resets_stride : nullptr;
    s.pairs_per_step = g.pairs_per_step;
    s.n_targets = g.n_targets;
    s.first_step = g.first_step;
    s.best = g.best + gcls_out_row(m, g.n_steps, c.H) * 2;
    s.dist = g.dist ? g.dist + gcls_out_row(m, g.n_steps, c.H) * c.B : nullptr;
    s.total = g.total;
    return s;
}

// grid (ceil(max_pairs / HTM_CLASSIFIER_PAIRS), n * H): step i of a learning call, every member's
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kgcls_sum(GClsDev gd, GClsStep gs, int i) {
    const int m = gcls_member((int)blockIdx.y, gd.c.H), h = gcls_horizon((int)blockIdx.y, gd.c.H);
    if (m >= gd.n) return;
    const ClsDev c = gcls_dev(gd, m);
    cls_sum_block(c, gcls_step(gs, c, m), h, gd.c.steps[h], i);
}

// the same grid, behind kgcls_sum of the same step
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kgcls_apply(GClsDev gd, GClsStep gs, int i) {
    const int m = gcls_member((int)blockIdx.y, gd.c.H), h = gcls_horizon((int)blockIdx.y, gd.c.H);
    if (m >= gd.n) return;
    const ClsDev c = gcls_dev(gd, m);
    cls_apply_block(c, gcls_step(gs, c, m), h, gd.c.steps[h], i);
}

// grid (ceil(pairs_per_step / HTM_CLASSIFIER_PAIRS), streams * n * H), n <= gcls_chunk(streams, H): steps [first, first + n) of a frozen
// call, every member's.  The accumulators f are [streams * n * H] rows: a block row's own.
__global__ __launch_bounds__(HTM_CLASSIFIER_THREADS) void kgcls_frozen(GClsDev gd, ClsFrozen f, GClsStep gs, int first, int n) {
    const int y = (int)blockIdx.y, h = gcls_horizon(y, gd.c.H), zi = gcls_frozen_step(y, gd.c.H, n), m = gcls_frozen_member(y, gd.c.H, n);
    if (m >= gd.n) return;
    const ClsDev c = gcls_dev(gd, m);
    cls_frozen_block(c, f, gcls_step(gs, c, m), h, zi, first, n);
}

// Pattern capture of a recorded group call (htm_set_group_run_active_cells): grid (blocks, B), block row y being member y of the
// group's tables -- its Dev, its record descriptor (whose slot names the row) and its capture descriptor.  Directly behind
// kgrp_rec_step of the step of parity p.  A member without rows, or a step outside the call's records, writes nothing.
__global__ __launch_bounds__(256) void kgcls_capture(const Dev *__restrict__ tab, int p, RecDev *const *__restrict__ recs, const ClsCapDev *__restrict__ caps) {
    if (!caps[blockIdx.y].rows) return;
    cls_capture_rows(tab[blockIdx.y], p, recs[blockIdx.y], caps[blockIdx.y]);
}

// the flagged members' histories emptied (flags null: every member's); a thread per member
__global__ __launch_bounds__(256) void kgcls_reset(int64_t *count, const int32_t *flags, int n) {
    const int m = (int)(blockIdx.x * 256 + threadIdx.x);
    if (m < n && (!flags || flags[m])) count[m] = 0;
}

#endif  // __HIPCC__
#endif
