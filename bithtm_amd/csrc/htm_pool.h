// Pooling links of region stacks (htm_pool_columns; include/bithtm_hip.h, DESIGN.md sections 14 and 29): the link between two
// regions that gives the upper one a decaying union of the lower one's columns.  bithtm_amd/pooling.py is the definition and the
// kernels below are held to it bit for bit.
//
//   per lower step, with the step's active columns A and its column prediction colpred:
//     P    = max(P - decay, 0)                                                  every column
//     P[A] = min(ceiling, P[A] + (prev[A] ? predicted_weight : active_weight))
//     prev = colpred
//   per window of `stride` steps: bank row = a bit for each of the union_bits columns of the largest P among those with P > 0,
//   ties at the cut to the lower column index.  A reset bit of a window clears P and prev before the window's first step.
//
// Three launches per batch of windows, none of which waits for another block:
//   k_pack_columns (htm_stack.h), stride 1, into the scratch: one bitmap row of W words per lower step.
//   kpool_scan     one thread per column, P and prev in registers from the state arrays at the start to the state arrays at the
//                  end.  The thread walks the steps in order, POOL_AHEAD rows of its bitmap word and its prediction word in
//                  flight (both addresses are known ahead), and at each window's end stores P as one byte of the window's snapshot
//                  row (consecutive threads, consecutive bytes).  Threads of the pad columns [C, 32 W) store 0 and touch no state.
//   kpool_select   one block per window: a 256-bin histogram of the snapshot row (a private one per wave: most positive columns
//                  share a few values), the cut value and how many columns AT the cut still win, then a second pass over the row
//                  (L2) that builds 16 bits per thread in column order -- with a prefix count of the columns at the cut across the
//                  block where not all of them win -- into the row's bitmap in LDS, which goes out with 16-byte stores, pad
//                  words included.  Rows outside the call's range keep their contents.
// The scratch of a batch of B windows: B * stride bitmap rows (W words each), then B snapshot rows (32 W bytes each).
// Served up to POOL_MAX_COLUMNS lower columns (the select's row bitmap and its histograms fit the LDS a launch gets without asking
// for more); above that the entry refuses.
#ifndef BITHTM_HTM_POOL_H
#define BITHTM_HTM_POOL_H

#define POOL_THREADS 256
#define POOL_WAVES (POOL_THREADS / 64)
#define POOL_AHEAD 8                        // rows a scan thread keeps in flight
#define POOL_TRIP (POOL_THREADS * 16)       // columns a select block covers per trip: 16 snapshot bytes per thread
#define POOL_MAX_COLUMNS (256 * 1024)       // 32 KiB of row bitmap + 4 KiB of histograms

struct PoolDev {
    int C, W, PW;                           // lower columns; words of a bitmap row (= the upper handle's words_per_row); words of a prediction row
    int stride, n_windows;
    int active_weight, predicted_weight, decay, ceiling, union_bits;
    int bank_rows, first_row;
    const uint32_t *bitmaps;                // [n_windows * stride][W]
    const uint32_t *colpred;                // [n_windows * stride][PW]
    const uint32_t *resets;                 // bit (first_row + r) % bank_rows: a reset before window r; or null
    uint8_t *persistence;                   // [C]
    uint32_t *prev;                         // [PW]
    uint8_t *snap;                          // [n_windows][32 W]
    uint32_t *bank;
};

static inline size_t pool_window_bytes(int W, int stride) { return (size_t)stride * (size_t)W * 4 + (size_t)W * 32; }
static inline size_t pool_select_lds(int W) { return (size_t)W * 4; }

#ifdef __HIPCC__

// A scan thread's work over the descriptor `a`, written once: kpool_scan below and the member-indexed kgpool_scan
// (htm_group_stack.h) call it.  (The select block's statements are htm_pool_select.inc, for the reason given there.)
__device__ __forceinline__ void pool_scan_thread(const PoolDev &a) {
    const int c = (int)(blockIdx.x * POOL_THREADS + threadIdx.x);
    const size_t pitch = (size_t)a.W * 32;
    if ((size_t)c >= pitch) return;
    uint8_t *snap = a.snap + c;
    if (c >= a.C) {                                                             // a pad column: zeros for the select's 16-byte loads
        for (int r = 0; r < a.n_windows; ++r) snap[(size_t)r * pitch] = 0;
        return;
    }
    const int word = c >> 5, sh = c & 31;
    int P = a.persistence[c];
    bool prev = (a.prev[word] >> sh) & 1u;
    const uint32_t *act = a.bitmaps + word, *pred = a.colpred + word;
    const long long n = (long long)a.n_windows * a.stride;
    int lj = 0, lrow = a.first_row;                                             // the loads' place: step of the window, bank row of the window
    int cj = 0, r = 0;                                                          // the arithmetic's place: step of the window, window
    for (long long s0 = 0; s0 < n; s0 += POOL_AHEAD) {
        uint32_t av[POOL_AHEAD], pv[POOL_AHEAD], rv[POOL_AHEAD];
#pragma unroll
        for (int u = 0; u < POOL_AHEAD; ++u) {
            const long long s = s0 + u;
            av[u] = pv[u] = rv[u] = 0u;
            if (s < n) {
                av[u] = act[(size_t)s * (size_t)a.W];
                pv[u] = pred[(size_t)s * (size_t)a.PW];
                if (lj == 0 && a.resets) rv[u] = (a.resets[lrow >> 5] >> (lrow & 31)) & 1u;     // (lrow < bank_rows)
                if (++lj == a.stride) {
                    lj = 0;
                    if (++lrow == a.bank_rows) lrow = 0;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < POOL_AHEAD; ++u) {
            if (s0 + u < n) {
                if (rv[u]) {
                    P = 0;
                    prev = false;
                }
                P = max(P - a.decay, 0);
                if ((av[u] >> sh) & 1u) P = min(a.ceiling, P + (prev ? a.predicted_weight : a.active_weight));
                prev = (pv[u] >> sh) & 1u;
                if (++cj == a.stride) {
                    cj = 0;
                    snap[(size_t)r * pitch] = (uint8_t)P;                       // (ceiling <= 255)
                    ++r;
                }
            }
        }
    }
    a.persistence[c] = (uint8_t)P;
    // the wave's 64 columns are two words of prev; the first lane of a word is a live column whenever any of its lanes is
    const unsigned long long m = __ballot(prev);
    const int lane = lane_id();
    if (lane == 0) a.prev[word] = (uint32_t)m;
    if (lane == 32) a.prev[word] = (uint32_t)(m >> 32);
}

__global__ __launch_bounds__(POOL_THREADS) void kpool_scan(PoolDev a) { pool_scan_thread(a); }

// grid = windows, POOL_THREADS threads, dynamic LDS = pool_select_lds(W): the row's bitmap
__global__ __launch_bounds__(POOL_THREADS) void kpool_select(PoolDev a) {
#include "htm_pool_select.inc"
}

#endif  // __HIPCC__
#endif
