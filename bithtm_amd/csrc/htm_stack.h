// Region stacks (htm_pack_columns; include/bithtm_hip.h): the link between two regions of a stack.
//
// A lower region's recorded run leaves sp_state.active_column of each of its steps in a device buffer (htm_run_recorded:
// int32[steps][k], ascending).  The upper region's run reads packed input rows from a device bank (htm_run).  This launch
// turns the one into the other:
//   bank row (first_row + r) % bank_rows = OR over j in [0, stride) of the bits lists[(r * stride + j) * k + 0..k)
// One block per output row:
//   1. the row's bitmap (W words = input_dim padded to 128 bits) is zeroed in LDS with 16-byte writes;
//   2. threads over the stride * k list entries of the row's window, consecutive threads on consecutive entries (they are
//      contiguous in memory: coalesced loads), each setting its bit with an LDS atomicOr -- an id outside [0, input_dim)
//      sets no bit and raises the sticky PACK_ERROR_BIT in the counter block;
//   3. the finished row goes out with 16-byte vector stores, pad words included: the block writes every word of its row
//      and nothing else, so the bank needs no memset and rows outside the call's range stay what they were.
// All LDS is the dynamic region (16-byte aligned base, no statics in front of it).
#ifndef BITHTM_HTM_STACK_H
#define BITHTM_HTM_STACK_H

#define PACK_THREADS 256
#define PACK_LDS_MAX (64 * 1024)          // a row of more bytes than this is refused (input_dim above 524 288), not given a second path
#define PACK_ERROR_BIT 64                 // Counters::error: a recorded column id outside the upper region's input range

static inline size_t pack_lds(const Dev &d) { return (size_t)d.W * 4; }

// The block's work on output row blockIdx.x of the handle `d`, written once: k_pack_columns below and the member-indexed
// kgrp_pack_columns (htm_group_stack.h) call it.  s_row: the launch's dynamic LDS, [d.W] words.
__device__ __forceinline__ void pack_columns_block(const Dev &d, const int32_t *__restrict__ lists, int32_t k, int32_t stride,
                                                   uint32_t *__restrict__ bank, int32_t bank_rows, int32_t first_row, uint32_t *s_row) {
    uint4 *s_row4 = reinterpret_cast<uint4 *>(s_row);
    for (int w = (int)threadIdx.x; w < d.W4; w += PACK_THREADS) s_row4[w] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const size_t r = blockIdx.x;
    const long long n = (long long)stride * k;                                  // entries of this row's window
    const int32_t *src = lists + r * (size_t)n;
    bool bad = false;
    for (long long i = threadIdx.x; i < n; i += PACK_THREADS) {
        const uint32_t id = (uint32_t)src[i];
        if (id < (uint32_t)d.I) atomicOr(&s_row[id >> 5], 1u << (id & 31));     // (id < I <= 32 W: inside the row)
        else bad = true;                                                        // (negative ids too: they compare as large)
    }
    if (bad) atomicOr(&d.ctr->error, PACK_ERROR_BIT);
    __syncthreads();
    const size_t row = (size_t)(((long long)first_row + (long long)r) % bank_rows);
    uint4 *dst = reinterpret_cast<uint4 *>(bank + row * (size_t)d.W);           // (rows are W words = 16 W4 bytes: aligned as the bank is)
    for (int w = (int)threadIdx.x; w < d.W4; w += PACK_THREADS) dst[w] = s_row4[w];
}

__global__ __launch_bounds__(PACK_THREADS) void k_pack_columns(Dev d, const int32_t *__restrict__ lists, int32_t k, int32_t stride,
                                                               uint32_t *__restrict__ bank, int32_t bank_rows, int32_t first_row) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_row[];            // [d.W], d.W = 4 * d.W4
    pack_columns_block(d, lists, k, stride, bank, bank_rows, first_row, s_row);
}

#endif
