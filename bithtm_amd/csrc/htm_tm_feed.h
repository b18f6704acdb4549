// Batched stand-alone Temporal Memory runs (htm_tm_run; include/bithtm_hip.h): the launch at the head of
// each step, which turns one row of a device bank of active-column lists into the step's sorted winner list.
//
// htm_tm_step sorts and checks the caller's list on the host and copies it over, once per step.  A run keeps the lists on the
// device: int32 [n_rows][n], each row n distinct column ids in any order.  Step t reads row t % n_rows, t being the handle's own
// step index, which the launch reads from the counter block -- so a graph captured for one parity replays for any step.
//
// All blocks first clear the parity's act / pred / win words and column bitmap, grid-stride, as k_tm_load_active does.  Block 0
// then sorts the row by counting through a column bitmap in LDS (the shape of k_pack_columns, htm_stack.h):
//   1. the bitmap (one bit per column, padded to 16 bytes) is zeroed with 16-byte writes;
//   2. threads over the row's n entries, consecutive threads on consecutive entries (coalesced loads), each setting its bit
//      with an LDS atomicOr; the returned word tells a repeated id, the range check an id outside [0, column_dim);
//   3. each thread counts the bits of its run of consecutive bitmap words, a block prefix sum gives the run's first slot, and
//      the thread emits its columns in ascending bit order to active_cols[p][slot...]: plain stores.
// No comparison network, and the row is validated in the same pass.
//
// A bad row (an id out of range, or twice) leaves fewer than n bits.  The launches behind this one take n by value and must
// find n distinct in-range ids, so thread 0 sets the lowest clear bits until n are set (column_dim >= n: there are enough), and
// raises the sticky FEED_ERROR_BIT in the counter block: the step ran on a list the caller did not give, its result is invalid,
// and htm_get_info reports it.  Nothing is read or written out of bounds either way: bits are only set below column_dim, and
// every emitted slot is checked against n.
//
// All LDS is the dynamic region (16-byte aligned base, no statics in front of it): the bitmap, then the block scan's wave sums
// and the block's bad-row flag.
#ifndef BITHTM_HTM_TM_FEED_H
#define BITHTM_HTM_TM_FEED_H

#define FEED_THREADS 256
#define FEED_LDS_MAX (64 * 1024)          // a column bitmap of more bytes than this is refused (column_dim above 524 032), not given a second path
#define FEED_ERROR_BIT 128                // Counters::error: a list row with a repeated column id or one outside [0, column_dim)

// 32-bit words of the column bitmap, padded to whole 16-byte groups
static inline int feed_words(const Dev &d) { return ((d.C + 31) / 32 + 3) & ~3; }
static inline size_t feed_bitmap_bytes(const Dev &d) { return (size_t)feed_words(d) * 4; }
static inline size_t feed_lds(const Dev &d) { return feed_bitmap_bytes(d) + 32; }      // (the bitmap, four wave sums, the bad-row flag)

__global__ __launch_bounds__(FEED_THREADS) void k_tm_feed(Dev d, int p, const int32_t *__restrict__ lists, int32_t n_rows, int32_t n) {
    for (int c = blockIdx.x * FEED_THREADS + threadIdx.x; c < d.C * d.WPC; c += gridDim.x * FEED_THREADS) {
        d.act[p][c] = 0;
        d.pred[p][c] = 0;
        d.win[p][c] = 0;
        if (c < d.colwords) d.colbits[p][c] = 0;
    }
    if (blockIdx.x != 0) return;
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[];           // [words], then the scan's four wave sums and the bad-row flag
    const int words = ((d.C + 31) / 32 + 3) & ~3, tid = (int)threadIdx.x;
    uint4 *s_bits4 = reinterpret_cast<uint4 *>(s_bits);
    uint32_t *s_wave = s_bits + words, *s_bad = s_wave + 4;
    for (int w = tid; w < words / 4; w += FEED_THREADS) s_bits4[w] = make_uint4(0u, 0u, 0u, 0u);
    if (tid == 0) *s_bad = 0u;
    __syncthreads();
    const int32_t *src = lists + (size_t)(d.ctr->step[p] % (uint32_t)n_rows) * (size_t)n;
    bool bad = false;
    for (int i = tid; i < n; i += FEED_THREADS) {
        const uint32_t id = (uint32_t)src[i];
        if (id < (uint32_t)d.C) {                                               // (id < C <= 32 * words: inside the bitmap)
            const uint32_t bit = 1u << (id & 31);
            if (atomicOr(&s_bits[id >> 5], bit) & bit) bad = true;              // listed twice
        } else {
            bad = true;                                                         // (negative ids too: they compare as large)
        }
    }
    if (bad) *s_bad = 1u;
    __syncthreads();
    if (*s_bad) {                                                               // (the same answer in every thread)
        if (tid == 0) {
            int have = 0;
            for (int w = 0; w < words; ++w) have += __popc(s_bits[w]);
            for (int c = 0; c < d.C && have < n; ++c)                           // the lowest columns not listed
                if (!((s_bits[c >> 5] >> (c & 31)) & 1u)) { s_bits[c >> 5] |= 1u << (c & 31); ++have; }
            atomicOr(&d.ctr->error, FEED_ERROR_BIT);
        }
        __syncthreads();
    }
    // runs of `per` consecutive words per thread (a multiple of four: one or more 16-byte reads), ascending with the thread index
    const int per = ((words + FEED_THREADS - 1) / FEED_THREADS + 3) & ~3, w0 = tid * per;
    uint32_t cnt = 0;
    for (int w = w0; w < min(w0 + per, words); w += 4) {
        const uint4 v = s_bits4[w >> 2];
        cnt += (uint32_t)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
    }
    uint32_t total;
    uint32_t slot = block_excl_scan<FEED_THREADS>(cnt, s_wave, total);
    int *out = d.active_cols[p];
    for (int w = w0; w < min(w0 + per, words) && cnt; ++w) {
        uint32_t m = s_bits[w];
        while (m) {
            const int b = __ffs((int)m) - 1;
            m &= m - 1u;
            if (slot < (uint32_t)n) out[slot] = w * 32 + b;                     // (total == n: always true; the store stays inside [0, n) regardless)
            ++slot;
        }
    }
}

// The record of a stand-alone Temporal Memory step (k_rec_step for a winner list of n <= active_columns entries): the record
// says n, and an active_column row holds the list in its first n of active_columns slots and -1 in the rest.
__global__ __launch_bounds__(256) void k_tm_feed_record(Dev d, int p, RecDev *r, int n) { role_rec_step(d, p, r, n); }

#endif
