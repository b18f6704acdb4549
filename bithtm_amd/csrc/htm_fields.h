// Field kinds of scalar streams (include/bithtm_hip.h): category fields and hashed (random distributed
// scalar) fields beside the linear ones of htm_scalar.h, in the same table.  bithtm_amd/encoders.py is the definition --
// CategoryField, HashedField -- and the kernels below are held to it bit for bit.
//
//   The kind travels in htm_scalar_field::reserved: 0 = linear (htm_scalar.h, unchanged), reserved & 3 = HTM_FIELD_CATEGORY or
//   HTM_FIELD_HASHED, reserved >> 2 = the seed of a hashed field.
//   category:  missing unless 0 <= floor((v - minimum) * scale) < buckets; bucket c owns the bits offset + c * width + j, j < width
//   hashed:    bucket(v) of a non-periodic linear field over `buckets` buckets; bucket b sets offset + pos(b + j), j < width,
//              pos(i) = (draw32(stream_base(seed, HTM_STREAM_FIELD_HASH, 0), i, 0) * bits) >> 32, i < buckets + width - 1;
//              decode: G[i] = votes[offset + pos(i)], score[b] = G[b] + ... + G[b + width - 1]
//
// A table whose fields are all linear launches k_bank_encode, k_decode_votes and klive_finish exactly as before (those kernels are
// not touched: their names and figures are pinned); a table with at least one other field launches the twins below at the same
// places with the same grids:
//   kenc_bank    k_bank_encode's contract -- one block per row, every word of the row written once in 16-byte stores, no
//                read-modify-write, no atomics.  Linear and category windows are bit ranges as there; the positions of a hashed
//                window (at most HTM_HASHED_MAX_WIDTH per field) are hashed once per row into LDS, and each storing thread ORs
//                in those that fall into its four words.
//   kenc_votes   k_decode_votes' contract, over role_field_votes: role_decode_votes with the scanned element votes[offset +
//                pos(i)] for a hashed field (pos hashed on the fly) and the window P[(c + 1) * width] - P[c * width] for a category.
//   kenc_finish  klive_finish's body over that role.
// (A table with a coordinate field -- kind HTM_FIELD_COORDINATE, a group of three entries -- launches the kernels of htm_coord.h
// instead, which are these with the coordinate kind added; field_elements and field_bucket below are never asked about that kind.)
// The arithmetic (field_kind, field_pos, field_bucket) is __host__ __device__ and this file can be included without hipcc -- after
// htm_rng.h, with __host__, __device__ and __forceinline__ defined away: tests/host_stub/field_kinds_host.cpp evaluates it on the
// host against the Python definition.  Part of the single translation unit htm_engine.hip (included after htm_live.h).
#ifndef BITHTM_HTM_FIELDS_H
#define BITHTM_HTM_FIELDS_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define FIELD_HD __host__ __device__ __forceinline__
#else
#define FIELD_HD static inline
#endif

FIELD_HD int field_kind(const htm_scalar_field &f) { return f.reserved & 3; }
FIELD_HD uint32_t field_seed(const htm_scalar_field &f) { return (uint32_t)f.reserved >> 2; }
FIELD_HD uint32_t field_hash_base(const htm_scalar_field &f) { return htm_stream_base(field_seed(f), HTM_STREAM_FIELD_HASH, 0u); }

// pos(i) of a hashed field of `bits` bits: in [0, bits)
FIELD_HD int field_pos(uint32_t base, uint32_t i, int bits) {
    return (int)(((uint64_t)htm_draw32(base, i, 0u) * (uint64_t)(uint32_t)bits) >> 32);
}

// how many elements the decode scans for a field: its bits, the bits its categories own, or the positions of a hashed field
FIELD_HD int field_elements(const htm_scalar_field &f) {
    const int kind = field_kind(f);
    return kind == HTM_FIELD_HASHED ? f.buckets + f.width - 1 : kind == HTM_FIELD_CATEGORY ? f.buckets * f.width : f.bits;
}

// bucket(v) of the definition, every kind (the linear cases as scalar_bucket of htm_scalar.h; a hashed field is never periodic)
FIELD_HD int field_bucket(const htm_scalar_field &f, double v) {
    const double d = v - f.minimum;
    const double t = d * f.scale;
    if (field_kind(f) == HTM_FIELD_CATEGORY) {
        const double c = floor(t);
        return c >= 0.0 && c < (double)f.buckets ? (int)c : -1;     // (NaN and +-inf fail the comparison; -0.0 is category 0)
    }
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

// whether a checked table holds a field that is not linear (the host's choice between the kernels of htm_scalar.h and the twins)
static inline bool fields_mixed(const htm_scalar_field *f, int n_fields) {
    for (int j = 0; j < n_fields; ++j)
        if (f[j].reserved != 0) return true;
    return false;
}

#ifdef __HIPCC__

// grid = rows, block = scalar_encode_threads(W).  Thread j < n_fields: the row's bucket of field j, and its window as bit ranges
// (linear, category) or as a count of hashed positions.  Then, per hashed field with a value, the block's threads hash its
// `width` positions into s_pos; then a thread per four words, as k_bank_encode.  Every loop bound is block-uniform (LDS words
// written before the barrier in front of it).  s_pos is 16 x 256 ints = 16 KiB.
__global__ __launch_bounds__(SCALAR_THREADS) void kenc_bank(Dev d, ScalarTab tab, int n_fields, const double *__restrict__ values,
                                                            uint32_t *__restrict__ bank, int first_row) {
    __shared__ int s_lo[HTM_SCALAR_MAX_FIELDS], s_hi[HTM_SCALAR_MAX_FIELDS], s_lo2[HTM_SCALAR_MAX_FIELDS], s_hi2[HTM_SCALAR_MAX_FIELDS];
    __shared__ int s_first[HTM_SCALAR_MAX_FIELDS], s_count[HTM_SCALAR_MAX_FIELDS];
    __shared__ int s_pos[HTM_SCALAR_MAX_FIELDS][HTM_HASHED_MAX_WIDTH];
    const int r = (int)blockIdx.x;
    if ((int)threadIdx.x < n_fields) {
        const int j = (int)threadIdx.x;
        const htm_scalar_field &f = tab.f[j];
        const int kind = field_kind(f);
        const int b = field_bucket(f, values[(size_t)r * n_fields + j]);
        int lo = 0, hi = 0, hi2 = 0, count = 0;
        if (b >= 0) {
            if (kind == HTM_FIELD_HASHED) {
                count = f.width;
            } else if (kind == HTM_FIELD_CATEGORY) {
                lo = b * f.width;
                hi = lo + f.width;
            } else {
                lo = b;
                hi = min(b + f.width, f.bits);
                hi2 = b + f.width - hi;             // (what wraps round the field's end: a periodic field only)
            }
        }
        s_lo[j] = f.offset + lo;
        s_hi[j] = f.offset + hi;
        s_lo2[j] = f.offset;
        s_hi2[j] = f.offset + hi2;
        s_first[j] = b;
        s_count[j] = count;
    }
    __syncthreads();
    for (int j = 0; j < n_fields; ++j) {
        const int count = s_count[j];
        if (count == 0) continue;
        const htm_scalar_field &f = tab.f[j];
        const uint32_t base = field_hash_base(f);
        const int b = s_first[j];
        for (int t = (int)threadIdx.x; t < count; t += (int)blockDim.x) s_pos[j][t] = f.offset + field_pos(base, (uint32_t)(b + t), f.bits);
    }
    __syncthreads();
    uint32_t *out = bank + (size_t)(first_row + r) * (size_t)d.W;
    for (int q = (int)threadIdx.x; q < (d.W >> 2); q += (int)blockDim.x) {      // four words = 128 inputs (W is a multiple of 4)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int j = 0; j < n_fields; ++j) {
            const int lo = s_lo[j], hi = s_hi[j], lo2 = s_lo2[j], hi2 = s_hi2[j], count = s_count[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int base = (4 * q + u) * 32;
                w[u] |= scalar_range_word(lo, hi, base) | scalar_range_word(lo2, hi2, base);
            }
            for (int t = 0; t < count; ++t) {       // (every lane reads the same LDS word: a broadcast)
                const int p = s_pos[j][t];
                const int word = (p >> 5) - 4 * q;
                const uint32_t bit = 1u << (p & 31);
#pragma unroll
                for (int u = 0; u < 4; ++u) w[u] |= word == u ? bit : 0u;
            }
        }
        *reinterpret_cast<uint4 *>(out + 4 * (size_t)q) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// role_decode_votes (htm_scalar.h) for a field of any kind: the same prefix array, scan and 64-bit max key.  What differs is
// the element fed to the scan -- votes[offset + pos(i)] for a hashed field -- how many there are (field_elements, at most
// HTM_DECODE_MAX_BITS: the host checks) and the window of a bucket in the prefix sums.  Every branch on the kind is block-uniform.
__device__ __forceinline__ void role_field_votes(const htm_scalar_field &f, const int32_t *__restrict__ votes, int32_t *__restrict__ o) {
    __shared__ uint32_t s_p[HTM_DECODE_MAX_BITS + 1];
    __shared__ uint32_t s_w[SCALAR_WAVES];
    __shared__ u64 s_k[SCALAR_WAVES];
    const int kind = field_kind(f), bits = f.bits, width = f.width, buckets = f.buckets;
    const int n = field_elements(f);
    const uint32_t base = field_hash_base(f);
    const int32_t *v = votes + f.offset;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) s_p[0] = 0u;
    uint32_t carry = 0u;
    for (int i0 = 0; i0 < n; i0 += SCALAR_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        uint32_t x = 0u;
        if (i < n) x = (uint32_t)v[kind == HTM_FIELD_HASHED ? field_pos(base, (uint32_t)i, bits) : i];
        const uint32_t incl = wave_incl_scan(x);
        if (lane == 63) s_w[wave] = incl;
        __syncthreads();
        uint32_t before = carry, total = 0u;
#pragma unroll
        for (int u = 0; u < SCALAR_WAVES; ++u) {
            const uint32_t t = s_w[u];
            before += u < wave ? t : 0u;
            total += t;
        }
        if (i < n) s_p[i + 1] = before + incl;
        carry += total;
        __syncthreads();                            // (s_w is written again in the next pass; s_p is read behind the last one)
    }
    u64 best = 0ull;                                // (score 0 with ~b = 0: below every key a thread forms)
    for (int b = (int)threadIdx.x; b < buckets; b += SCALAR_THREADS) {
        uint32_t score;
        if (kind == HTM_FIELD_CATEGORY) {
            score = s_p[(b + 1) * width] - s_p[b * width];
        } else if (kind == HTM_FIELD_HASHED) {
            score = s_p[b + width] - s_p[b];
        } else {
            const int e = b + width;
            score = s_p[min(e, bits)] - s_p[b];
            if (e > bits) score += s_p[e - bits];   // (a periodic window past the field's end: P[0] = 0)
        }
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

// grid x = row, y = field, SCALAR_THREADS threads: k_decode_votes over role_field_votes
__global__ __launch_bounds__(SCALAR_THREADS) void kenc_votes(ScalarTab tab, int n_fields, int I, const int32_t *__restrict__ votes,
                                                             int32_t *__restrict__ out) {
    role_field_votes(tab.f[blockIdx.y], votes + (size_t)blockIdx.x * (size_t)I, out + ((size_t)blockIdx.x * n_fields + blockIdx.y) * 2);
}

// klive_finish (htm_live.h) over role_field_votes: grid (max(n_fields, 1), B) behind step p's record and votes launches
__global__ __launch_bounds__(SCALAR_THREADS) void kenc_finish(const Dev *__restrict__ tab, int p, ScalarTab ftab, int n_fields,
                                                              const int32_t *__restrict__ votes, const htm_step_record *__restrict__ recs,
                                                              htm_live_row *__restrict__ rows, int32_t *__restrict__ pairs) {
    const int i = (int)blockIdx.y;
    const Dev &d = tab[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        htm_live_row r;
        r.record = recs[i];
        r.step_index = (int64_t)d.ctr->step[p];
        r.capacity_error = d.ctr->error;
        r.reserved = 0;
        rows[i] = r;
    }
    if ((int)blockIdx.x < n_fields)
        role_field_votes(ftab.f[blockIdx.x], votes + (size_t)i * (size_t)d.I, pairs + ((size_t)i * n_fields + blockIdx.x) * 2);
}

#endif  // __HIPCC__
#endif
