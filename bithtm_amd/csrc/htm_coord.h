// Coordinate fields of scalar streams (include/bithtm_hip.h): a 2-D integer position and a radius in, the
// `width` cells of the square round the position that a keyed hash ranks highest out, each as one bit of the field.  Positions
// that are close share most of their cells' bits, positions more than two radii apart share none but by chance.
// bithtm_amd/encoders.py (CoordinateField) is the definition and the kernels below are held to it bit for bit.
//
//   A field is three consecutive table entries, one per value column: the head (kind HTM_FIELD_COORDINATE, bits >= 1: the x
//   column, buckets = max_radius, reserved >> 2 = the seed), and two continuations (kind HTM_FIELD_COORDINATE, bits 0: the y and
//   the radius column) -- the host checks the layout (scalar_table).
//   cell(v)     t = (v - minimum) * scale; missing unless -2^30 <= t < 2^30; else (int32)floor(t)
//   radius(v)   t = (v - minimum) * scale; missing if NaN or t < 0; else (int)min(floor(t), (double)max_radius)
//   candidates  the N = (2r + 1)^2 cells of [cx - r, cx + r] x [cy - r, cy + r], index i = (y - (cy - r)) * (2r + 1) + (x - (cx - r))
//   order(x, y) = draw24(stream_base(seed, HTM_STREAM_COORDINATE, 0), x, y);  bit(x, y) = (draw32(stream_base(seed, .., 1), x, y) * bits) >> 32
//   the row gets offset + bit(p) of the min(width, N) candidates p of the largest order, ties at the cut to the lower index
//
// A table with a coordinate field launches the three kernels below where a mixed table launches the twins of htm_fields.h:
//   kcoord_bank    kenc_bank's contract and body, on SCALAR_THREADS threads whatever the row's width (the select wants them), plus,
//                  per coordinate field with a value, a select in LDS (coord_select) that appends the winners' bit positions to the
//                  field's s_pos slots.
//   kcoord_votes   kenc_votes, kcoord_finish: kenc_finish -- a block whose entry is of the coordinate kind writes (-1, 0) and leaves
//                  (there is no decode: what a bit says about the position is not recoverable).
// The arithmetic (coord_cell, coord_radius, coord_order, coord_bit) is __host__ __device__ and this file can be included without
// hipcc, behind htm_rng.h and htm_fields.h: tests/host_stub/coordinate_host.cpp evaluates it on the host.  Part of the single
// translation unit htm_engine.hip (included after htm_fields.h).
#ifndef BITHTM_HTM_COORD_H
#define BITHTM_HTM_COORD_H

#include <math.h>
#include <stdint.h>

FIELD_HD bool coord_head(const htm_scalar_field &f) { return field_kind(f) == HTM_FIELD_COORDINATE && f.bits >= 1; }
FIELD_HD bool coord_tail(const htm_scalar_field &f) { return field_kind(f) == HTM_FIELD_COORDINATE && f.bits < 1; }
FIELD_HD uint32_t coord_order_base(uint32_t seed) { return htm_stream_base(seed, HTM_STREAM_COORDINATE, 0u); }
FIELD_HD uint32_t coord_bit_base(uint32_t seed) { return htm_stream_base(seed, HTM_STREAM_COORDINATE, 1u); }

// the cell of an axis: false for a missing value (NaN and +-inf fail the comparison)
FIELD_HD bool coord_cell(const htm_scalar_field &f, double v, int32_t *cell) {
    const double d = v - f.minimum;
    const double t = d * f.scale;
    if (!(t >= -1073741824.0 && t < 1073741824.0)) return false;
    *cell = (int32_t)floor(t);
    return true;
}

// the radius in cells, clamped to max_radius in double and then converted; -1 for a missing value
FIELD_HD int coord_radius(const htm_scalar_field &f, double v, int max_radius) {
    const double d = v - f.minimum;
    const double t = d * f.scale;
    if (t != t || t < 0.0) return -1;
    const double c = floor(t), top = (double)max_radius;
    return (int)(c > top ? top : c);
}

FIELD_HD uint32_t coord_order(uint32_t base, int32_t x, int32_t y) { return htm_draw24(base, (uint32_t)x, (uint32_t)y); }
FIELD_HD int coord_bit(uint32_t base, int32_t x, int32_t y, int bits) {
    return (int)(((uint64_t)htm_draw32(base, (uint32_t)x, (uint32_t)y) * (uint64_t)(uint32_t)bits) >> 32);
}

// whether a checked table holds a coordinate field (the host's choice of kernels: this first, then fields_mixed)
static inline bool fields_coordinate(const htm_scalar_field *f, int n_fields) {
    for (int j = 0; j < n_fields; ++j)
        if ((f[j].reserved & 3) == HTM_FIELD_COORDINATE) return true;
    return false;
}

#ifdef __HIPCC__

#define COORD_DIGITS 256                    // an 8-bit digit of the 24-bit order per pass: three passes, most significant first

// The select of one coordinate field of one row, by the whole block (SCALAR_THREADS threads); every argument is block-uniform,
// and so is every loop bound and branch.  Writes min(width, N) positions offset + bit(p) to pos[] and returns how many.
//   N <= width: every candidate, no select.
//   else three histogram passes over the order's digits, most significant first, among the candidates that agree with the digits
//   found so far: the digit in whose bin the width-th largest order falls, and how many of that bin are still wanted.  Behind
//   the third pass `cut` is the order of the last winner and `want` how many candidates of exactly that order win (at least 1).
//   Then one pass that appends every candidate above the cut, and of those AT the cut the `want` of the lowest index: where all
//   of them win (a cut without a tie, nearly always) in any order, else in index order, SCALAR_THREADS candidates per round with
//   a ballot count per wave and a running total.
// The orders are hashed again in every pass (two mix32 each, no memory).  s_hist, s_scan and s_sel are the caller's LDS.
__device__ __forceinline__ int coord_select(const htm_scalar_field &f, int32_t cx, int32_t cy, int r, int *pos, uint32_t *s_hist, uint32_t *s_scan,
                                            uint32_t *s_sel) {
    const int side = 2 * r + 1, N = side * side, width = f.width, bits = f.bits;
    const uint32_t seed = field_seed(f), obase = coord_order_base(seed), bbase = coord_bit_base(seed);
    const int32_t x0 = cx - r, y0 = cy - r;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    if (N <= width) {
        for (int i = tid; i < N; i += SCALAR_THREADS) pos[i] = f.offset + coord_bit(bbase, x0 + i % side, y0 + i / side, bits);
        return N;
    }
    uint32_t prefix = 0u, mask = 0u, want = (uint32_t)width, ties = 0u;
    for (int shift = 16; shift >= 0; shift -= 8) {
        s_hist[tid] = 0u;                           // (SCALAR_THREADS == COORD_DIGITS)
        __syncthreads();
        for (int i = tid; i < N; i += SCALAR_THREADS) {
            const uint32_t o = coord_order(obase, x0 + i % side, y0 + i / side);
            if ((o & mask) == prefix) atomicAdd(&s_hist[(o >> shift) & 255u], 1u);
        }
        __syncthreads();
        // thread t looks at digit 255 - t: `incl` candidates have that digit or a larger one
        const uint32_t mine = s_hist[COORD_DIGITS - 1 - tid];
        const uint32_t scan = wave_incl_scan(mine);
        if (lane == 63) s_scan[wave] = scan;
        __syncthreads();
        uint32_t incl = scan;
#pragma unroll
        for (int u = 0; u < SCALAR_WAVES; ++u) incl += u < wave ? s_scan[u] : 0u;
        if (incl - mine < want && want <= incl) {   // (exactly one thread: the bins together hold at least `want`)
            s_sel[0] = (uint32_t)(COORD_DIGITS - 1 - tid);
            s_sel[1] = want - (incl - mine);
            s_sel[2] = mine;
        }
        __syncthreads();
        prefix |= s_sel[0] << shift;
        mask |= 255u << shift;
        want = s_sel[1];
        ties = s_sel[2];
        __syncthreads();                            // (s_hist, s_scan and s_sel are written again in the next pass)
    }
    const uint32_t cut = prefix;
    if (tid == 0) s_sel[0] = 0u;                    // the slots taken
    __syncthreads();
    if (want == ties) {
        for (int i = tid; i < N; i += SCALAR_THREADS) {
            const int32_t x = x0 + i % side, y = y0 + i / side;
            if (coord_order(obase, x, y) >= cut) {
                const uint32_t slot = atomicAdd(&s_sel[0], 1u);
                if (slot < (uint32_t)width) pos[slot] = f.offset + coord_bit(bbase, x, y, bits);
            }
        }
    } else {
        uint32_t seen = 0u;                         // candidates at the cut below this round's
        for (int i0 = 0; i0 < N; i0 += SCALAR_THREADS) {
            const int i = i0 + tid;
            const int32_t x = x0 + i % side, y = y0 + i / side;
            const uint32_t o = i < N ? coord_order(obase, x, y) : 0u;
            const bool at = i < N && o == cut;
            const unsigned long long m = __ballot(at);
            if (lane == 0) s_scan[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = seen, total = 0u;
#pragma unroll
            for (int u = 0; u < SCALAR_WAVES; ++u) {
                const uint32_t t = s_scan[u];
                before += u < wave ? t : 0u;
                total += t;
            }
            const uint32_t rank = before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if ((i < N && o > cut) || (at && rank < want)) {
                const uint32_t slot = atomicAdd(&s_sel[0], 1u);
                if (slot < (uint32_t)width) pos[slot] = f.offset + coord_bit(bbase, x, y, bits);
            }
            seen += total;
            __syncthreads();                        // (s_scan is written again in the next round)
        }
    }
    __syncthreads();
    return width;
}

// grid = rows, SCALAR_THREADS threads: kenc_bank with the coordinate kind.  Thread j < n_fields prepares entry j as there; the thread
// of a coordinate head reads the three values of its group and leaves the centre and the radius (-1: a missing value, no bit) in
// LDS, a continuation leaves empty ranges.  Then the hashed windows, then a select per coordinate field with a value, then the
// stores.  s_pos is 16 x 256 ints = 16 KiB, the select's words 1 KiB.
__global__ __launch_bounds__(SCALAR_THREADS) void kcoord_bank(Dev d, ScalarTab tab, int n_fields, const double *__restrict__ values,
                                                              uint32_t *__restrict__ bank, int first_row) {
    __shared__ int s_lo[HTM_SCALAR_MAX_FIELDS], s_hi[HTM_SCALAR_MAX_FIELDS], s_lo2[HTM_SCALAR_MAX_FIELDS], s_hi2[HTM_SCALAR_MAX_FIELDS];
    __shared__ int s_first[HTM_SCALAR_MAX_FIELDS], s_count[HTM_SCALAR_MAX_FIELDS], s_cy[HTM_SCALAR_MAX_FIELDS], s_r[HTM_SCALAR_MAX_FIELDS];
    __shared__ int s_pos[HTM_SCALAR_MAX_FIELDS][HTM_HASHED_MAX_WIDTH];
    __shared__ uint32_t s_hist[COORD_DIGITS], s_scan[SCALAR_WAVES], s_sel[4];
    static_assert(COORD_DIGITS == SCALAR_THREADS, "coord_select clears and scans a bin per thread");
    const int r = (int)blockIdx.x;
    if ((int)threadIdx.x < n_fields) {
        const int j = (int)threadIdx.x;
        const htm_scalar_field &f = tab.f[j];
        const int kind = field_kind(f);
        const double *v = values + (size_t)r * n_fields + j;
        int lo = 0, hi = 0, hi2 = 0, count = 0, first = -1, cy = 0, radius = -1;
        if (kind == HTM_FIELD_COORDINATE) {
            if (f.bits >= 1) {                      // (a head: entries j + 1 and j + 2 are its continuations -- the host checks)
                int32_t cx = 0, c2 = 0;
                const bool okx = coord_cell(f, v[0], &cx), oky = coord_cell(tab.f[j + 1], v[1], &c2);
                const int rr = coord_radius(tab.f[j + 2], v[2], f.buckets);
                if (okx && oky && rr >= 0) {
                    first = cx;
                    cy = c2;
                    radius = rr;
                }
            }
        } else {
            const int b = field_bucket(f, v[0]);
            first = b;
            if (b >= 0) {
                if (kind == HTM_FIELD_HASHED) {
                    count = f.width;
                } else if (kind == HTM_FIELD_CATEGORY) {
                    lo = b * f.width;
                    hi = lo + f.width;
                } else {
                    lo = b;
                    hi = min(b + f.width, f.bits);
                    hi2 = b + f.width - hi;         // (what wraps round the field's end: a periodic field only)
                }
            }
        }
        s_lo[j] = f.offset + lo;
        s_hi[j] = f.offset + hi;
        s_lo2[j] = f.offset;
        s_hi2[j] = f.offset + hi2;
        s_first[j] = first;
        s_count[j] = count;
        s_cy[j] = cy;
        s_r[j] = radius;
    }
    __syncthreads();
    for (int j = 0; j < n_fields; ++j) {
        const htm_scalar_field &f = tab.f[j];
        if (field_kind(f) == HTM_FIELD_COORDINATE) {
            const int radius = s_r[j];
            if (radius < 0) continue;
            const int count = coord_select(f, s_first[j], s_cy[j], radius, s_pos[j], s_hist, s_scan, s_sel);
            if (threadIdx.x == 0) s_count[j] = count;
            continue;
        }
        const int count = s_count[j];
        if (count == 0) continue;
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

// grid x = row, y = field, SCALAR_THREADS threads: kenc_votes; an entry of the coordinate kind decodes to (-1, 0)
__global__ __launch_bounds__(SCALAR_THREADS) void kcoord_votes(ScalarTab tab, int n_fields, int I, const int32_t *__restrict__ votes,
                                                               int32_t *__restrict__ out) {
    int32_t *o = out + ((size_t)blockIdx.x * n_fields + blockIdx.y) * 2;
    if (field_kind(tab.f[blockIdx.y]) == HTM_FIELD_COORDINATE) {
        if (threadIdx.x == 0) {
            o[0] = -1;
            o[1] = 0;
        }
        return;
    }
    role_field_votes(tab.f[blockIdx.y], votes + (size_t)blockIdx.x * (size_t)I, o);
}

// kenc_finish with the same addition: grid (max(n_fields, 1), B) behind step p's record and votes launches
__global__ __launch_bounds__(SCALAR_THREADS) void kcoord_finish(const Dev *__restrict__ tab, int p, ScalarTab ftab, int n_fields,
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
    if ((int)blockIdx.x >= n_fields) return;
    int32_t *o = pairs + ((size_t)i * n_fields + blockIdx.x) * 2;
    if (field_kind(ftab.f[blockIdx.x]) == HTM_FIELD_COORDINATE) {
        if (threadIdx.x == 0) {
            o[0] = -1;
            o[1] = 0;
        }
        return;
    }
    role_field_votes(ftab.f[blockIdx.x], votes + (size_t)i * (size_t)d.I, o);
}

#endif  // __HIPCC__
#endif
