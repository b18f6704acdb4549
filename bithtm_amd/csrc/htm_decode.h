// Predicted-input decoding (htm_predicted_input, htm_set_run_predicted_input; include/bithtm_hip.h).
//
// The votes of a state are the top-down pass of the Spatial Pooler's proximal projection over the columns the state predicts:
//   votes[i] = #{ columns c : any cell of c predicted (pred[q], networks.py:30-33,122), mask[c] bit i (permanence >= threshold,
//                 projections.py:18-21) }
// int32[input_dim], one launch.  Blocks over chunks of PIN_COLS columns, and in each block:
//   1. every thread tests PIN_COLS / 256 columns (the WPC prediction words of each, all loads issued together) and appends the
//      predicted ones to a list in LDS -- the test of rec_column_bits;
//   2. threads over input bits, PIN_BITS consecutive bits each (one mask word holds all of them): for every listed column the
//      thread loads its mask word, PIN_UNROLL columns' loads issued together, and counts its bits in registers;
//   3. one atomic per non-zero count per block, into the output row, which the caller has zeroed.
// A block without a predicted column returns after step 1.  The launch reads pred, mask and the step counter and writes only
// its output row: it can follow any launch that has finished a step.
#ifndef BITHTM_HTM_DECODE_H
#define BITHTM_HTM_DECODE_H

#define PIN_COLS 1024
#define PIN_BITS 4
#define PIN_UNROLL 8

// device-side descriptor of the current decoding call (one per handle; graphs of decoding steps hold its address, the call's
// k_pin_begin fills it)
struct PinDev {
    int32_t *out;              // [n][I] or null
    uint32_t base;             // step index of row 0
    int32_t n;                 // rows of this call
};

// blocks of a decoding launch over C columns
static inline int pin_blocks(int C) { return (C + PIN_COLS - 1) / PIN_COLS; }

// the votes of parity q's prediction words, added into out[0, I) (zeroed by the caller)
__device__ __forceinline__ void role_pin(const Dev &d, int q, int32_t *__restrict__ out) {
    __shared__ int s_list[PIN_COLS];
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int c_first = (int)(blockIdx.x * PIN_COLS + threadIdx.x);
    uint32_t any[PIN_COLS / 256];
#pragma unroll
    for (int u = 0; u < PIN_COLS / 256; ++u) {
        const int c = c_first + u * 256;
        uint32_t a = 0;
        if (c < d.C) {
            a = d.pred[q][(size_t)c * d.WPC];
            if (d.WPC == 2) a |= d.pred[q][(size_t)c * 2 + 1];
        }
        any[u] = a;
    }
#pragma unroll
    for (int u = 0; u < PIN_COLS / 256; ++u)
        if (any[u]) s_list[atomicAdd(&s_n, 1)] = c_first + u * 256;       // (at most PIN_COLS entries: one per column of the chunk)
    __syncthreads();
    const int n = s_n;
    if (n == 0) return;                               // (the same answer in every thread of the block)
    for (int i0 = (int)threadIdx.x * PIN_BITS; i0 < d.I; i0 += 256 * PIN_BITS) {
        const uint32_t *m = d.mask + (i0 >> 5);      // (i0 < I <= 32 W: inside the row)
        const int sh = i0 & 31;
        uint32_t cnt[PIN_BITS] = {};
        for (int j = 0; j < n; j += PIN_UNROLL) {
            uint32_t w[PIN_UNROLL];
#pragma unroll
            for (int u = 0; u < PIN_UNROLL; ++u) w[u] = j + u < n ? m[(size_t)s_list[j + u] * d.W] : 0u;
#pragma unroll
            for (int u = 0; u < PIN_UNROLL; ++u) {
                const uint32_t bits = w[u] >> sh;
#pragma unroll
                for (int r = 0; r < PIN_BITS; ++r) cnt[r] += (bits >> r) & 1u;
            }
        }
#pragma unroll
        for (int r = 0; r < PIN_BITS; ++r)
            if (cnt[r] && i0 + r < d.I) atomicAdd(out + i0 + r, (int32_t)cnt[r]);
    }
}

// htm_predicted_input: the votes of the last completed step (parity q) into out (zeroed just before)
__global__ __launch_bounds__(256) void k_pin(Dev d, int q, int32_t *out) { role_pin(d, q, out); }

// Before a decoding call's first step: its rows zeroed (grid-stride) and the descriptor filled
__device__ __forceinline__ void role_pin_begin(PinDev *r, int32_t *out, uint32_t base, int32_t n, int I) {
    if (out) {
        const size_t total = (size_t)n * I, stride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) out[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r->out = out;
        r->base = base;
        r->n = out ? n : 0;
    }
}

__global__ __launch_bounds__(256) void k_pin_begin(PinDev *r, int32_t *out, uint32_t base, int32_t n, int I) {
    role_pin_begin(r, out, base, n, I);
}

// Behind step p's last launch, beside k_rec_step: row ctr->step[p] - base of the call's output, nothing outside [base, base + n)
__device__ __forceinline__ void role_pin_step(const Dev &d, int p, const PinDev *r) {
    const uint32_t slot = d.ctr->step[p] - r->base;
    if (slot >= (uint32_t)r->n) return;
    role_pin(d, p, r->out + (size_t)slot * d.I);
}

__global__ __launch_bounds__(256) void k_pin_step(Dev d, int p, const PinDev *r) { role_pin_step(d, p, r); }

// model groups (htm_group.h): grid y = member, each member's own descriptor and output (null: nothing decoded).  Row 0 is the
// member's next step: the index the last completed step -- parity q -- left in the counter block, as kgrp_rec_begin takes it.
__global__ __launch_bounds__(256) void kgrp_pin_begin(const Dev *__restrict__ tab, int q, PinDev *const *__restrict__ pins,
                                                      int32_t *const *__restrict__ outs, int32_t n) {
    const Dev &d = tab[blockIdx.y];
    role_pin_begin(pins[blockIdx.y], outs[blockIdx.y], d.ctr->step[q ^ 1], n, d.I);
}

__global__ __launch_bounds__(256) void kgrp_pin_step(const Dev *__restrict__ tab, int p, PinDev *const *__restrict__ pins) {
    role_pin_step(tab[blockIdx.y], p, pins[blockIdx.y]);
}

#endif
