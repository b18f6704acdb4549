// Device-side input noise (htm_bank_noise; include/bithtm_hip.h): the keyed flip noise of the example's
// loop, `pattern ^ (np.random.rand(input_dim) < p)` (example.py:52), with np.random.rand replaced by keyed stream 6.
//
//   flip(seed, step)[i] = i < input_dim  and  draw24(stream_base(seed, HTM_STREAM_INPUT_NOISE, step), i, 0) < threshold24
//   dst row (step % n_dst) = src row (step % n_src) ^ flip(seed, step)        for step = first_step + r, r in [0, n_rows)
// with `step` a uint32 that wraps as the device's step counter does.  threshold24 = ceil(p * 2^24) is formed on the host, so
// that the integer comparison is the float one (m * 2^-24 < p) for every m in [0, 2^24).
//
// A bulk fill, one block per row.  The row is W words = input_dim padded to 128 bits; a wave takes 64 consecutive inputs at a
// time, lane l drawing for input 64 c + l, and the ballot of the comparison is the two flip words of that chunk (as role_encode,
// htm_forecast.h).  Lane 0 XORs them with the chunk's two source words and writes the pair with one 8-byte store.  Inputs at
// and above input_dim never flip and the source's pad bits are 0, so the pad bits stay 0 whatever the threshold; every word
// of a written row is written (no memset), and rows outside the window are not touched.
//
// Where the uint32 step wraps inside the window two of its steps can land in one row of the ring (2^32 is no multiple of
// n_dst).  The later step then owns the row, as in the sequential loop of the definition; the block of the earlier one returns.
//
// Reset bits: behind the row blocks come blocks with one thread per 32-bit word of the ring's reset bits (bit j: a reset before
// the step that reads ring row j, htm_reset.h).  A thread forms its whole word -- for a row inside the window the source flag
// of the step that owns the row (bit step % n_src of src_resets), for a row outside it 0 -- and writes it with one store: no
// read-modify-write, and no bit of an earlier window survives.
#ifndef BITHTM_HTM_NOISE_H
#define BITHTM_HTM_NOISE_H

#define NOISE_THREADS 256
#define NOISE_WAVES (NOISE_THREADS / 64)

static inline int noise_reset_blocks(int n_dst) { return ((n_dst + 31) / 32 + NOISE_THREADS - 1) / NOISE_THREADS; }

// The window's step that owns ring row j: its offset r in [0, n_rows), or -1 for a row outside the window.  k = the steps of the
// window before the uint32 wrap (n_rows: no wrap inside it)
__device__ __forceinline__ int noise_row_owner(uint32_t j, uint32_t first_step, int n_rows, uint32_t n_dst, uint32_t k) {
    if (k + (u64)j < (u64)n_rows) return (int)(k + j);            // behind the wrap: step j, in row j (j < n_rows <= n_dst)
    const uint32_t r = (j + n_dst - first_step % n_dst) % n_dst;     // before it: the rows run on from first_step % n_dst
    return r < k ? (int)r : -1;
}

__global__ __launch_bounds__(NOISE_THREADS) void k_bank_noise(Dev d, const uint32_t *__restrict__ src, int32_t n_src, uint32_t *__restrict__ dst,
                                                              int32_t n_dst, uint32_t first_step, int32_t n_rows, uint32_t seed,
                                                              uint32_t threshold24, const uint32_t *__restrict__ src_resets,
                                                              uint32_t *__restrict__ dst_resets) {
    const u64 to_wrap = 0x100000000ull - (u64)first_step;
    const uint32_t k = to_wrap < (u64)n_rows ? (uint32_t)to_wrap : (uint32_t)n_rows;
    if ((int)blockIdx.x >= n_rows) {                                // the reset words (launched only with reset pointers)
        const int w = ((int)blockIdx.x - n_rows) * NOISE_THREADS + (int)threadIdx.x;
        if (w >= (n_dst + 31) / 32) return;
        uint32_t word = 0;
        for (int b = 0; b < 32; ++b) {
            const uint32_t j = (uint32_t)w * 32u + (uint32_t)b;
            if (j >= (uint32_t)n_dst) break;
            const int r = noise_row_owner(j, first_step, n_rows, (uint32_t)n_dst, k);
            if (r < 0) continue;
            const uint32_t row = (first_step + (uint32_t)r) % (uint32_t)n_src;
            word |= ((src_resets[row >> 5] >> (row & 31)) & 1u) << b;
        }
        dst_resets[w] = word;
        return;
    }
    const uint32_t r = blockIdx.x;
    const uint32_t step = first_step + r;                           // (wraps as the device's step counter does)
    const uint32_t slot = step % (uint32_t)n_dst;
    if (r < k && k + (u64)slot < (u64)n_rows) return;              // a step behind the wrap owns this row
    const uint32_t base = htm_stream_base(seed, HTM_STREAM_INPUT_NOISE, step);
    const uint32_t *in = src + (size_t)(step % (uint32_t)n_src) * (size_t)d.W;
    uint32_t *out = dst + (size_t)slot * (size_t)d.W;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    for (int c = wave; c < (d.W >> 1); c += NOISE_WAVES) {          // 64 inputs = two words (W is a multiple of 4)
        const int i = c * 64 + lane;
        const u64 m = __ballot(i < d.I && htm_draw24(base, (uint32_t)i, 0u) < threshold24);
        if (lane == 0) {
            const uint2 x = *reinterpret_cast<const uint2 *>(in + 2 * (size_t)c);      // (rows are 16-byte aligned)
            *reinterpret_cast<uint2 *>(out + 2 * (size_t)c) = make_uint2(x.x ^ (uint32_t)m, x.y ^ (uint32_t)(m >> 32));
        }
    }
}

#endif
