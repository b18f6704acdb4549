// Anomaly likelihood on the device (htm_likelihood_*, include/bithtm_hip.h; the definition is
// bithtm_amd/likelihood.py, which this file equals bit for bit).  Per stream the device keeps t (scores seen), the ring of the last
// averaging_window raw scores q, the ring of the last `history` short-term averages a (both indexed by absolute step modulo
// their length), and the current estimate (mean, std) with a flag.  One role serves every caller:
//   role_likelihood(state of one stream, records, n_steps <= HTM_LIKELIHOOD_CHUNK, out)
// run by one block of 256 threads per stream (grid y = stream), so nothing is shared between blocks and no atomics are needed.
//   1  every thread takes two steps of the chunk: q from the record's two counts, then a from the up to 64 values of q that end
//      at its step (the chunk's in LDS and, below the chunk's start, the carried ring's)
//   2  if a re-estimation point falls inside the chunk (their positions are in closed form from t): the prefix sums of a and
//      a*a over the chunk, and over the ring entries that leave the window while the chunk passes, and the window's sums at the
//      chunk's start, all int64 in LDS.  Integer sums are associative: a window's (N, S1, S2) as differences of these equals
//      the sequential loop's.
//   3  every step finds the point that governs it (the latest one <= t, in the chunk; else the carried estimate, or none), forms
//      that point's (mean, std) from the prefix sums and writes L_t as a float64 with a plain vector store
//   4  behind a barrier (phases 1 and 2 read ring entries that are overwritten here): the chunk's last `history` values of a and
//      last averaging_window values of q go into the rings, t advances, and the estimate governing the last step is kept
// The float64 arithmetic is in the three functions below, each operation a single IEEE operation in the order the definition
// has them (the translation unit is compiled with -ffp-contract=off, as htm_fexp.h needs it); the Gaussian tail is a table of 513
// doubles the host builds and hands over as data.  The functions are __host__ __device__ and the file can be included without
// HIP: tests/host_stub/likelihood_host.cpp evaluates them on the host against the definition.
// Part of the single translation unit htm_engine.hip (included after htm_live.h).
#ifndef BITHTM_HTM_LIKELIHOOD_H
#define BITHTM_HTM_LIKELIHOOD_H

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LIK_HD __host__ __device__
#else
#define LIK_HD
#endif

#define HTM_LIKELIHOOD_CHUNK 512            // steps per launch (bithtm_amd/_lib.py: LIKELIHOOD_CHUNK)
#define HTM_LIKELIHOOD_THREADS 256          // two steps per thread
#define HTM_LIKELIHOOD_TAIL 513             // entries of the tail table: TAIL[i] = 0.5 * erfc((i / 64) / sqrt 2)
#define HTM_LIKELIHOOD_MAX_HISTORY 16384
#define HTM_LIKELIHOOD_MAX_WINDOW 64

// the raw score of a step in units of 2^-16: (bursting << 16) // active, 0 without active columns
LIK_HD static inline int32_t lik_q_of(int32_t active, int32_t bursting) {
    return active > 0 ? (int32_t)(((uint64_t)(uint32_t)bursting << 16) / (uint32_t)active) : 0;
}

// (mean, std) of a window from its exact count, sum and sum of squares (n * s2 and s1 * s1 stay below 2^63: n <= 2^14, a <= 2^16)
LIK_HD static inline void lik_estimate(int64_t n, int64_t s1, int64_t s2, double *mean, double *std) {
    const double m = (double)s1 / (double)n;
    const double v = (double)(n * s2 - s1 * s1) / (double)(n * n);
    *mean = m > 1966.08 ? m : 1966.08;                      // 0.03 in units of 2^-16
    *std = sqrt(v > 1288490.1888 ? v : 1288490.1888);       // 0.0003 in units of 2^-32
}

// L of the short-term average a under (mean, std): the tail table interpolated linearly at min(|z|, 8) * 64
LIK_HD static inline double lik_likelihood(int32_t a, double mean, double std, const double *tail) {
    const double z = ((double)a - mean) / std;
    const double az = fabs(z);
    const double x = (az < 8.0 ? az : 8.0) * 64.0;
    int i = (int)x;
    if (i > 511) i = 511;
    const double f = x - (double)i;
    const double t0 = tail[i];
    const double d = tail[i + 1] - t0;
    const double p = f * d;
    const double t = t0 + p;
    return z < 0 ? t : 1.0 - t;
}

#ifdef __HIPCC__

struct LikParams {
    int32_t learning_period, estimation_samples, history, window, reestimation_period;
};

// the device state of n streams, the parts of ONE allocation in the order htm_likelihood_export documents
struct LikDev {
    LikParams p;
    int64_t *t;                 // [n]
    double *mean, *std;         // [n]
    int32_t *flag;              // [n]   1: (mean, std) is an estimate
    int32_t *q_ring;            // [n][window]
    int32_t *a_ring;            // [n][history]
    const double *tail;         // [513]
};

// Inclusive scan of one (v1, v2) pair per thread over the block's 256 threads -> the thread's EXCLUSIVE prefixes in v1, v2 and the
// block's totals.  Every thread of the block calls it (it has barriers); s1, s2: 256 int64 of LDS each, free for reuse afterwards.
__device__ inline void lik_block_scan(int64_t &v1, int64_t &v2, int64_t *s1, int64_t *s2, int64_t &total1, int64_t &total2) {
    const int tid = (int)threadIdx.x;
    s1[tid] = v1;
    s2[tid] = v2;
    __syncthreads();
    for (int off = 1; off < HTM_LIKELIHOOD_THREADS; off <<= 1) {
        const int64_t a1 = tid >= off ? s1[tid - off] : 0, a2 = tid >= off ? s2[tid - off] : 0;
        __syncthreads();
        s1[tid] += a1;
        s2[tid] += a2;
        __syncthreads();
    }
    const int64_t i1 = s1[tid], i2 = s2[tid];
    total1 = s1[HTM_LIKELIHOOD_THREADS - 1];
    total2 = s2[HTM_LIKELIHOOD_THREADS - 1];
    __syncthreads();
    v1 = i1 - v1;
    v2 = i2 - v2;
}

// Steps [0, n) of stream s, n in [1, HTM_LIKELIHOOD_CHUNK]: recs[j] is step j's record, out[j] its likelihood.  Called by every
// thread of a 256-thread block; s and n are block-uniform.  Every index below is bounded by n, the stream's own ring lengths or the
// LDS arrays' sizes: ring indices are reduced modulo the ring's length, prefix indices lie in [0, n].
__device__ inline void role_likelihood(const LikDev &L, int s, const htm_step_record *__restrict__ recs, int n, double *__restrict__ out) {
    constexpr int CH = HTM_LIKELIHOOD_CHUNK, W = HTM_LIKELIHOOD_MAX_WINDOW;
    __shared__ int32_t qs[W + CH];              // q of the W steps below the chunk (0 where there is none), then the chunk's
    __shared__ int64_t c1[CH + 1], c2[CH + 1];  // c[j] = sum of a (a*a) over the chunk's steps [0, j)
    __shared__ int64_t d1[CH], d2[CH];          // d[m] = sum of a (a*a) over the ring's steps [lo0, lo0 + m)
    __shared__ int64_t sc1[HTM_LIKELIHOOD_THREADS], sc2[HTM_LIKELIHOOD_THREADS];
    const int tid = (int)threadIdx.x;
    const LikParams p = L.p;
    const int w = p.window, hist = p.history;
    const int64_t t0 = L.t[s];
    int32_t *__restrict__ qr = L.q_ring + (size_t)s * (size_t)w;
    int32_t *__restrict__ ar = L.a_ring + (size_t)s * (size_t)hist;
    const int carried_flag = L.flag[s];
    const double carried_mean = L.mean[s], carried_std = L.std[s];
    const int rq0 = (int)(t0 % w), ra0 = (int)(t0 % hist);

    // ---- 1: q, then a
    if (tid < W) {
        const int m = tid + 1;                  // step t0 - m, needed for m < w
        int32_t v = 0;
        if (m < w && t0 - m >= 0) {
            int idx = rq0 - m;
            if (idx < 0) idx += w;
            v = qr[idx];
        }
        qs[W - m] = v;
    }
    _Pragma("unroll") for (int e = 0; e < 2; ++e) {
        const int j = 2 * tid + e;
        int32_t q = 0;
        if (j < n) {
            const htm_step_record r = recs[j];
            q = lik_q_of(r.active_columns, r.bursting_columns);
        }
        qs[W + j] = q;
    }
    __syncthreads();
    int32_t a_mine[2];
    _Pragma("unroll") for (int e = 0; e < 2; ++e) {
        const int j = 2 * tid + e;
        int32_t a = 0;
        if (j < n) {
            const int64_t seen = t0 + j + 1;
            const int count = seen < w ? (int)seen : w;
            int32_t sum = 0;
            for (int m = 0; m < count; ++m) sum += qs[W + j - m];
            a = sum / count;
        }
        a_mine[e] = a;
    }

    // ---- 2: the prefix sums, if a re-estimation point lies in the chunk (block-uniform)
    const int64_t probation = (int64_t)p.learning_period + p.estimation_samples;
    const int64_t u0 = t0 + 1 - probation;      // step j is a point iff u0 + j >= 0 and (u0 + j) % reestimation_period == 0
    int64_t um = u0 % p.reestimation_period;    // u0 modulo the period, in [0, period) also for a negative u0
    if (um < 0) um += p.reestimation_period;
    const int64_t first_point = u0 <= 0 ? -u0 : (um ? p.reestimation_period - um : 0);
    const bool has_point = first_point < n;
    int64_t lo0 = t0 + 1 - hist;                // the window's first step at the chunk's first step
    if (lo0 < p.learning_period) lo0 = p.learning_period;
    const int64_t ring_n = t0 > lo0 ? t0 - lo0 : 0;         // ring steps [lo0, t0) of that window: at most history - 1
    const int rl0 = (int)(lo0 % hist);
    int64_t ring1 = 0, ring2 = 0;               // their sums
    if (has_point) {
        int64_t v1 = (int64_t)a_mine[0] + a_mine[1], v2 = (int64_t)a_mine[0] * a_mine[0] + (int64_t)a_mine[1] * a_mine[1];
        int64_t x1, x2;
        lik_block_scan(v1, v2, sc1, sc2, x1, x2);
        c1[2 * tid] = v1;
        c2[2 * tid] = v2;
        c1[2 * tid + 1] = v1 + a_mine[0];
        c2[2 * tid + 1] = v2 + (int64_t)a_mine[0] * a_mine[0];
        if (tid == HTM_LIKELIHOOD_THREADS - 1) { c1[CH] = x1; c2[CH] = x2; }
        // the ring entries that leave the window while the chunk passes: the first min(ring_n, CH) of its steps
        int32_t g[2];
        _Pragma("unroll") for (int e = 0; e < 2; ++e) {
            const int m = 2 * tid + e;
            int32_t v = 0;
            if (m < ring_n) {
                int idx = rl0 + m;              // (m < CH: reduced with % -- history may be smaller than the chunk)
                idx %= hist;
                v = ar[idx];
            }
            g[e] = v;
        }
        v1 = (int64_t)g[0] + g[1];
        v2 = (int64_t)g[0] * g[0] + (int64_t)g[1] * g[1];
        lik_block_scan(v1, v2, sc1, sc2, x1, x2);
        d1[2 * tid] = v1;
        d2[2 * tid] = v2;
        d1[2 * tid + 1] = v1 + g[0];
        d2[2 * tid + 1] = v2 + (int64_t)g[0] * g[0];
        // ... and all of them
        v1 = v2 = 0;
        for (int64_t m = tid; m < ring_n; m += HTM_LIKELIHOOD_THREADS) {
            int idx = rl0 + (int)m;             // (both below history)
            if (idx >= hist) idx -= hist;
            const int64_t v = ar[idx];
            v1 += v;
            v2 += v * v;
        }
        lik_block_scan(v1, v2, sc1, sc2, ring1, ring2);
    }
    __syncthreads();

    // ---- 3: every step's governing estimate and its likelihood
    int last_flag = carried_flag;
    double last_mean = carried_mean, last_std = carried_std;
    _Pragma("unroll") for (int e = 0; e < 2; ++e) {
        const int j = 2 * tid + e;
        if (j >= n) break;
        int have = carried_flag;
        double mean = carried_mean, std = carried_std;
        const int64_t uj = u0 + j;
        if (uj >= 0) {
            const int back = (int)((um + j) % p.reestimation_period);
            const int jp = j - back;            // the latest point <= this step, as a step of the chunk
            if (jp >= 0) {
                const int64_t tp = t0 + jp;
                int64_t lo = tp + 1 - hist;
                if (lo < p.learning_period) lo = p.learning_period;
                const int64_t cnt = tp + 1 - lo;
                const int from = lo > t0 ? (int)(lo - t0) : 0;
                int64_t s1 = c1[jp + 1] - c1[from], s2 = c2[jp + 1] - c2[from];
                if (lo < t0) {
                    const int gone = (int)(lo - lo0);       // (<= jp < n, and < ring_n)
                    s1 += ring1 - d1[gone];
                    s2 += ring2 - d2[gone];
                }
                lik_estimate(cnt, s1, s2, &mean, &std);
                have = 1;
            }
        }
        out[j] = have ? lik_likelihood(a_mine[e], mean, std, L.tail) : 0.5;
        if (j == n - 1) { last_flag = have; last_mean = mean; last_std = std; }
    }

    // ---- 4: the rings, t and the estimate
    __syncthreads();
    _Pragma("unroll") for (int e = 0; e < 2; ++e) {
        const int j = 2 * tid + e;
        if (j >= n) break;
        if (j >= n - hist) ar[(ra0 + j) % hist] = a_mine[e];
        if (j >= n - w) qr[(rq0 + j) % w] = qs[W + j];
        if (j == n - 1) {
            L.t[s] = t0 + n;
            L.flag[s] = last_flag;
            L.mean[s] = last_mean;
            L.std[s] = last_std;
        }
    }
}

// grid (1, streams): steps [first, first + n) of a call of `total` steps per stream; stream s reads tab[s] (one: the only stream's
// records, by value, when tab is null) and writes out[s][first ..]
__global__ __launch_bounds__(HTM_LIKELIHOOD_THREADS) void klik_update(LikDev L, const htm_step_record *const *__restrict__ tab,
                                                                      const htm_step_record *__restrict__ one, int first, int n, int total,
                                                                      double *__restrict__ out) {
    const int s = (int)blockIdx.y;
    const htm_step_record *recs = tab ? tab[s] : one;
    role_likelihood(L, s, recs + first, n, out + (size_t)s * (size_t)total + first);
}

// grid (1, B), behind a live tick's record launches: member s's record slot recs[s] is its stream's next step
__global__ __launch_bounds__(HTM_LIKELIHOOD_THREADS) void klik_tick(LikDev L, const htm_step_record *__restrict__ recs, double *__restrict__ out) {
    const int s = (int)blockIdx.y;
    role_likelihood(L, s, recs + s, 1, out + s);
}

// grid (1, streams): the streams whose flag is set (flags null: all) go back to t = 0 with empty rings and no estimate
__global__ __launch_bounds__(HTM_LIKELIHOOD_THREADS) void klik_reset(LikDev L, const int32_t *__restrict__ flags) {
    const int s = (int)blockIdx.y;
    if (flags && !flags[s]) return;
    for (int i = (int)threadIdx.x; i < L.p.history; i += HTM_LIKELIHOOD_THREADS) L.a_ring[(size_t)s * L.p.history + i] = 0;
    for (int i = (int)threadIdx.x; i < L.p.window; i += HTM_LIKELIHOOD_THREADS) L.q_ring[(size_t)s * L.p.window + i] = 0;
    if (threadIdx.x == 0) {
        L.t[s] = 0;
        L.flag[s] = 0;
        L.mean[s] = 0.0;
        L.std[s] = 0.0;
    }
}

#endif  // __HIPCC__
#endif
