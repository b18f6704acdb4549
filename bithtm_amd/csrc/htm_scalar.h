// Scalar streams (htm_bank_encode, htm_decode_votes, htm_predicted_value; include/bithtm_hip.h): values
// in, bank rows out; votes in, a bucket and a score per field out.  The reference has no encoder, so the definition is this
// project's own -- bithtm_amd/encoders.py is its NumPy form, and the two kernels below are held to it bit for bit.
//
//   A field (htm_scalar_field) owns the input bits [offset, offset + bits) and sets `width` of them per value.
//   buckets = bits for a periodic field, else bits - width + 1;  scale = buckets / (maximum - minimum), formed ONCE on the host
//   in float64 and handed over as that double, so both sides multiply by the same number.
//
//   bucket(v):  t = (v - minimum) * scale -- two separately rounded IEEE double operations (no a * b + c shape: nothing to
//               contract, and the library is built with -ffp-contract=off all the same)
//     non-periodic: a NaN t is missing (-1); else floor(t) clamped to [0, buckets - 1] IN DOUBLE and then converted, so +-inf and
//               huge values land on the end buckets and v == maximum on the last one
//     periodic: unless -2^31 <= t < 2^31 the value is missing (NaN and +-inf fail the comparison); else (int64)floor(t) mod
//               buckets, non-negative
//   encode:     a bucket b >= 0 sets the bits offset + (b + j) % bits, j < width (a non-periodic field never wraps); a missing
//               value sets no bit of its field
//   decode:     score[b] = sum of votes[offset + (b + j) % bits], j < width, for b in [0, buckets); the result is the lowest b
//               with the largest score, or (-1, 0) where that score is 0.  Votes are counts (never negative); scores are int32.
// The value of a bucket, minimum + (b + 0.5) / scale, is formed on the host from the bucket: the device never forms it, so
// there is no tolerance anywhere.
//
// k_bank_encode -- a bulk fill shaped like k_bank_noise (htm_noise.h), one block per row; the block has as many waves as the row
// has 16-byte stores for, one to four (scalar_encode_threads: a row of the bench shape is eight stores, one wave).  The first n_fields threads compute
// the row's buckets once and leave each field's window as two global bit ranges in LDS ([lo, hi) and the wrapped part [lo2,
// hi2), empty ranges as lo == hi).  Then a thread per four words: a word is the OR, over the fields, of the intersection of the
// ranges with the word's 32 inputs, and the four go out in one 16-byte store (rows are 16-byte aligned, W is a multiple of 4).
// Every word of a written row is written, pad words as zeros (a field never reaches past input_dim: the host checks); no
// read-modify-write, no atomics, no memset; rows outside the window are not touched.
//
// k_decode_votes -- grid x = row, y = field.  The block forms P[i] = votes[0] + ... + votes[i - 1] of its field in LDS, SCALAR_THREADS
// votes per pass (a wave scan, the waves' totals through LDS, a running carry), so P[0 .. bits] takes bits + 1 words: the cap
// HTM_DECODE_MAX_BITS = 8 192 bits per field is 32 KiB + 4 bytes of the block's static LDS.  Vote rows are input_dim int32 apart
// and field offsets arbitrary, so the loads are plain 4-byte ones.  Then threads over buckets: score[b] = P[min(b + width, bits)]
// - P[b], plus P[b + width - bits] where a periodic window wraps, and the 64-bit key (score << 32) | ~b under a max -- the
// largest score, and among equals the lowest b -- reduced over the wave (wave_reduce64) and the waves.  Thread 0 writes the two
// int32 (bucket, score) of out[row][field].  The prefix sums wrap like int32 arithmetic; differences are exact while the true
// score fits an int32 (the Python layer refuses column_dim * width >= 2^31).
#ifndef BITHTM_HTM_SCALAR_H
#define BITHTM_HTM_SCALAR_H

#define SCALAR_THREADS 256
#define SCALAR_WAVES (SCALAR_THREADS / 64)

// threads of k_bank_encode's block for rows of W words: a thread per 16-byte store, in whole waves, at most SCALAR_THREADS
static inline int scalar_encode_threads(int W) { return std::min(SCALAR_THREADS, ((W >> 2) + 63) / 64 * 64); }

// the field table, by value in the kernel arguments (16 x 40 bytes)
struct ScalarTab {
    htm_scalar_field f[HTM_SCALAR_MAX_FIELDS];
};

// bucket(v) of the definition
__device__ __forceinline__ int scalar_bucket(const htm_scalar_field &f, double v) {
    const double d = v - f.minimum;
    const double t = d * f.scale;
    if (f.periodic) {
        if (!(t >= -2147483648.0 && t < 2147483648.0)) return -1;
        long long b = (long long)floor(t) % (long long)f.buckets;
        if (b < 0) b += f.buckets;
        return (int)b;
    }
    if (t != t) return -1;
    double c = floor(t);
    const double top = (double)(f.buckets - 1);
    c = c < 0.0 ? 0.0 : c;
    c = c > top ? top : c;
    return (int)c;
}

// the bits of [lo, hi) that fall into the word of the inputs [base, base + 32)
__device__ __forceinline__ uint32_t scalar_range_word(int lo, int hi, int base) {
    const int a = max(lo, base) - base, e = min(hi, base + 32) - base;
    if (e <= a) return 0u;
    const uint32_t run = e - a == 32 ? 0xFFFFFFFFu : (1u << (e - a)) - 1u;
    return run << a;
}

__global__ __launch_bounds__(SCALAR_THREADS) void k_bank_encode(Dev d, ScalarTab tab, int n_fields, const double *__restrict__ values,
                                                                uint32_t *__restrict__ bank, int first_row) {
    __shared__ int s_lo[HTM_SCALAR_MAX_FIELDS], s_hi[HTM_SCALAR_MAX_FIELDS], s_lo2[HTM_SCALAR_MAX_FIELDS], s_hi2[HTM_SCALAR_MAX_FIELDS];
    const int r = (int)blockIdx.x;
    if ((int)threadIdx.x < n_fields) {
        const int j = (int)threadIdx.x;
        const htm_scalar_field &f = tab.f[j];
        const int b = scalar_bucket(f, values[(size_t)r * n_fields + j]);
        int lo = 0, hi = 0, hi2 = 0;
        if (b >= 0) {
            lo = b;
            hi = min(b + f.width, f.bits);
            hi2 = b + f.width - hi;                 // (what wraps round the field's end: a periodic field only)
        }
        s_lo[j] = f.offset + lo;
        s_hi[j] = f.offset + hi;
        s_lo2[j] = f.offset;
        s_hi2[j] = f.offset + hi2;
    }
    __syncthreads();
    uint32_t *out = bank + (size_t)(first_row + r) * (size_t)d.W;
    for (int q = (int)threadIdx.x; q < (d.W >> 2); q += (int)blockDim.x) {      // four words = 128 inputs (W is a multiple of 4)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < n_fields; ++j) {
            const int lo = s_lo[j], hi = s_hi[j], lo2 = s_lo2[j], hi2 = s_hi2[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int base = (4 * q + u) * 32;
                w[u] |= scalar_range_word(lo, hi, base) | scalar_range_word(lo2, hi2, base);
            }
        }
        *reinterpret_cast<uint4 *>(out + 4 * (size_t)q) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// the decode of one field of one vote row (votes: the row's first vote, the field's offset not yet added) into o[0] = bucket,
// o[1] = score: the body of k_decode_votes, which the finish launch of a model group's live tick (htm_live.h) runs per member
// and field
__device__ __forceinline__ void role_decode_votes(const htm_scalar_field &f, const int32_t *__restrict__ votes, int32_t *__restrict__ o) {
    __shared__ uint32_t s_p[HTM_DECODE_MAX_BITS + 1];
    __shared__ uint32_t s_w[SCALAR_WAVES];
    __shared__ u64 s_k[SCALAR_WAVES];
    const int bits = f.bits, width = f.width, buckets = f.buckets;
    const int32_t *v = votes + f.offset;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) s_p[0] = 0u;
    uint32_t carry = 0u;
    for (int i0 = 0; i0 < bits; i0 += SCALAR_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        const uint32_t incl = wave_incl_scan(i < bits ? (uint32_t)v[i] : 0u);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = 0u;
#pragma unroll
        for (int u = 0; u < SCALAR_WAVES; ++u) {
            const uint32_t t = s_w[u];
            before += u < wave ? t : 0u;
            total += t;
        }
        if (i < bits) s_p[i + 1] = before + incl;
        carry += total;
        __syncthreads();                            // (s_w is written again in the next pass; s_p is read behind the last one)
    }
    u64 best = 0ull;                                // (score 0 with ~b = 0: below every key a thread forms)
    for (int b = (int)threadIdx.x; b < buckets; b += SCALAR_THREADS) {
        const int e = b + width;
        uint32_t score = s_p[min(e, bits)] - s_p[b];
        if (e > bits) score += s_p[e - bits];       // (a periodic window past the field's end: P[0] = 0)
        const u64 key = ((u64)score << 32) | (u64)(uint32_t)~(uint32_t)b;
        best = key > best ? key : best;
    }
    best = wave_reduce64(best, 0ull, [](u64 a, u64 b) { return a > b ? a : b; });
    if (lane == 0) s_k[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int u = 1; u < SCALAR_WAVES; ++u) best = s_k[u] > best ? s_k[u] : best;
        const int32_t score = (int32_t)(best >> 32);
        o[0] = score > 0 ? (int32_t)~(uint32_t)best : -1;
        o[1] = score > 0 ? score : 0;
    }
}

__global__ __launch_bounds__(SCALAR_THREADS) void k_decode_votes(ScalarTab tab, int n_fields, int I, const int32_t *__restrict__ votes,
                                                                 int32_t *__restrict__ out) {
    role_decode_votes(tab.f[blockIdx.y], votes + (size_t)blockIdx.x * (size_t)I, out + ((size_t)blockIdx.x * n_fields + blockIdx.y) * 2);
}

#endif
