// Banks of KNN classifiers on the device (htm_knns_*, include/bithtm_hip.h; the definition is
// bithtm_amd/knn.py's KNNBankDefinition).  One object holds n stores, member-major -- pairs [n][capacity][max_pairs], labels and stamps
// [n][capacity] -- and the scratch of an update: the overlaps [n][chunk][capacity] of 16 bits each and, where a table does not fit
// LDS, the dense query tables [n][chunk][words].  The streams' counts and the one step total are the host's; an update hands the
// kernels one table of n input pointers and n (count before, count after) pairs, copied once.
//
// Every kernel here is a one-stream body of htm_knn.h given its member's offsets: the member is blockIdx.y (place: blockIdx.x), or
// blockIdx.y / the query groups in the distance launch, whose x runs over the slot blocks of the LARGEST count -- a block past its own
// stream's count leaves at once.  No block waits for another, nothing is accumulated across blocks, every sum is an integer.
// The chunk -- query steps per launch -- is the largest power of two <= HTM_KNN_CHUNK whose scratch fits HTM_KNNS_SCRATCH_BYTES and
// whose n x chunk fits a grid's y; the arithmetic is in the __host__ __device__ functions at the top.
// Part of the single translation unit htm_engine.hip (included after htm_knn.h).
#ifndef BITHTM_HTM_KNN_BANK_H
#define BITHTM_HTM_KNN_BANK_H

#include <stdint.h>

#include "htm_knn.h"

#define HTM_KNNS_SCRATCH_BYTES (256ll << 20)    // the most scratch a bank's update may hold (bithtm_amd/_lib.py: KNNS_SCRATCH_BYTES)
#define HTM_KNNS_MAX_STREAMS 65535              // a grid's y, at chunk 1
#define HTM_KNNS_GRID_Y 65535

// the scratch of an update of n streams at `chunk` query steps per launch, in bytes
CLS_HD static inline int64_t gknn_scratch_bytes(int64_t n, int64_t chunk, int64_t capacity, int64_t words) {
    return n * chunk * (capacity * 2 + (knn_in_lds(words) ? 0 : words * 4));
}
// query steps per launch: the largest power of two <= HTM_KNN_CHUNK that fits the budget and the grid; 0: not even one step fits
CLS_HD static inline int gknn_chunk(int64_t n, int64_t capacity, int64_t words) {
    for (int chunk = HTM_KNN_CHUNK; chunk >= 1; chunk >>= 1)
        if (gknn_scratch_bytes(n, chunk, capacity, words) <= HTM_KNNS_SCRATCH_BYTES && n * chunk <= HTM_KNNS_GRID_Y) return chunk;
    return 0;
}
// ... of a bank whose n streams share one store (one flat batch of queries, one set of scratch rows): the chunk of ONE stream under the
// same budget (0: not even one query fits), doubled from HTM_KNN_CHUNK on while it is below n and its scratch still fits -- a tick's n
// queries are then one launch
CLS_HD static inline int gknn_shared_chunk(int64_t n, int64_t capacity, int64_t words) {
    int chunk = gknn_chunk(1, capacity, words);
    while (chunk >= HTM_KNN_CHUNK && chunk < n && chunk * 2 <= 32768 && gknn_scratch_bytes(1, chunk * 2, capacity, words) <= HTM_KNNS_SCRATCH_BYTES) chunk *= 2;
    return chunk;
}
// member m's first element in an array of `per` elements per member
CLS_HD static inline int64_t gknn_offset(int64_t m, int64_t per) { return m * per; }
// y of the distance launch: the members' query groups, member-major
CLS_HD static inline int gknn_distance_rows(int n, int nq, int queries) { return n * knn_query_groups(nq, queries); }

#ifdef __HIPCC__

struct GKnnDev {
    KnnDev d;                   // member 0's arrays
    int32_t n, chunk;
};

// a call's inputs: s as the one-stream call has it, with member 0's labels, best and votes (the members' lie n_labels, n_steps x 5
// and n_steps x labels words apart); the members' pairs and counts come from the table
struct GKnnStep {
    KnnStep s;
    const ClsPair *const *pairs;    // [n]: each member's [n_steps][pairs_per_step]; null: s.pairs is member 0's and the members'
    int64_t pairs_stride;           //      lie pairs_stride pairs apart (a tick's captured rows)
    const int32_t *counts;          // [n][2]: the slots in use before and behind the call's append
    int32_t *pos;                   // [n][n_steps]: the slot of every step (null in a call that stores nothing)
};

__device__ __forceinline__ KnnDev gknn_member(const GKnnDev &g, int m) {
    KnnDev d = g.d;
    d.store += gknn_offset(m, (int64_t)d.capacity * d.max_pairs);
    d.label += gknn_offset(m, d.capacity);
    d.stamp += gknn_offset(m, d.capacity);
    d.ovl += gknn_offset(m, (int64_t)g.chunk * d.capacity);
    if (d.table) d.table += gknn_offset(m, (int64_t)g.chunk * d.words);
    return d;
}

__device__ __forceinline__ KnnStep gknn_member(const GKnnDev &g, const GKnnStep &gs, int m) {
    KnnStep s = gs.s;
    s.pairs = gs.pairs ? gs.pairs[m] : s.pairs + gknn_offset(m, gs.pairs_stride);
    if (s.labels) s.labels += gknn_offset(m, s.n_labels);
    s.best += gknn_offset(m, (int64_t)s.n_steps * 5);
    if (s.votes) s.votes += gknn_offset(m, (int64_t)s.n_steps * g.d.labels);
    s.count0 = gs.counts[2 * m];
    s.count = gs.counts[2 * m + 1];
    return s;
}

// grid n: block m prefix-sums its stream's label flags (a stream that stores nothing: every pos -1)
__global__ __launch_bounds__(256) void kgknn_place(GKnnDev g, GKnnStep gs) {
    const int m = (int)blockIdx.x;
    knn_place_block(gknn_member(g, m), gknn_member(g, gs, m), gs.pos + gknn_offset(m, gs.s.n_steps));
}

// grid (pair blocks of n_steps x max_pairs, n)
__global__ __launch_bounds__(256) void kgknn_append(GKnnDev g, GKnnStep gs) {
    const int m = (int)blockIdx.y;
    const KnnStep s = gknn_member(g, gs, m);
    if (s.count == s.count0) return;
    knn_append_pair(gknn_member(g, m), s, gs.pos + gknn_offset(m, s.n_steps), (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// grid (pair blocks of nq x pairs_per_step, n); a stream with an empty store has nothing in its tables
__global__ __launch_bounds__(256) void kgknn_scatter(GKnnDev g, GKnnStep gs, int first, int nq, int fill) {
    const int m = (int)blockIdx.y;
    const KnnStep s = gknn_member(g, gs, m);
    if (s.count == 0) return;
    knn_scatter_pair(gknn_member(g, m), s, first, nq, fill, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

template <bool TABLE_IN_LDS>
__device__ __forceinline__ void gknn_distance_block(const GKnnDev &g, const GKnnStep &gs, int first, int nq, uint32_t *lds) {
    const int groups = knn_query_groups(nq, g.d.queries);
    const int m = (int)blockIdx.y / groups, by = (int)blockIdx.y % groups;
    const KnnStep s = gknn_member(g, gs, m);
    if (knn_block_first((int)blockIdx.x) >= s.count) return;        // (block-uniform: past this stream's count)
    knn_distance_block<TABLE_IN_LDS>(gknn_member(g, m), s, first, nq, lds, (int)blockIdx.x, by);
}

// grid (knn_slot_blocks(the largest count), gknn_distance_rows(n, nq, queries)), dynamic LDS knn_distance_lds(words) bytes
__global__ __launch_bounds__(256) void kgknn_distance_lds(GKnnDev g, GKnnStep gs, int first, int nq) {
    extern __shared__ uint32_t knn_tables[];
    gknn_distance_block<true>(g, gs, first, nq, knn_tables);
}

// the same grid, between kgknn_scatter(fill) and kgknn_scatter(clear) of the chunk
__global__ __launch_bounds__(256) void kgknn_distance_global(GKnnDev g, GKnnStep gs, int first, int nq) {
    extern __shared__ uint32_t knn_tables[];
    gknn_distance_block<false>(g, gs, first, nq, knn_tables);
}

// grid (nq, n): block (q, m) selects for member m's query first + q
__global__ __launch_bounds__(256) void kgknn_select(GKnnDev g, GKnnStep gs, int first) {
    const int m = (int)blockIdx.y;
    knn_select_block(gknn_member(g, m), gknn_member(g, gs, m), first, (int)blockIdx.x);
}

#endif  // __HIPCC__
#endif
