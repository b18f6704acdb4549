// Stream forks (htm_view_sync, htm_bank_rows; include/bithtm_hip.h): one handle's stream state copied into
// an inference view of the same weights, on the device, in one launch.
//
// The host hands k_stream_fork a small table by value (48 entries of 40 bytes: 1.9 KB of the launch's arguments): one entry per buffer of alloc_stream_state that is stream state (which,
// and why the others are not: DESIGN.md section 19), each (dst, src, bytes, kind, first block, blocks).  A block finds its entry
// by its index (a scan of at most FORK_MAX_ENTRIES scalars), then the block group of that entry strides over the entry's
// 16-byte vectors; the up to 15 bytes behind the last whole vector go byte by byte (the tail: one thread each, first block of the
// group).  No LDS, no scratch: the table is read from the kernel's arguments.
//
// Three kinds of entries.  FORK_FIXED: all `bytes` are copied.  FORK_ROWS (seg_info, seg_jit: a word per segment): the words of
// the segments below the SOURCE's Counters::S, read on the device -- the host does not know the count without waiting for the
// stream, and does not wait.  FORK_BITS (the match bits: a bit per segment): the words that hold a bit below S are copied, all
// words behind them up to the bitmap's capacity are ZEROED: whatever an earlier, longer-lived state of the view had set there
// reads "not matching" afterwards (the source's own bits at and above S are clear: every scan writes bits of rows below S only,
// and the import that lowers S rewrites the whole bitmap).
//
// The counter block goes with the launch (its first block, one thread per word): the source's, with the learning role's counts
// and the sticky capacity flags clear, as htm_create_view leaves them.
#ifndef BITHTM_HTM_FORK_H
#define BITHTM_HTM_FORK_H

#define FORK_THREADS 256
#define FORK_MAX_ENTRIES 48
#define FORK_VECS_PER_THREAD 8            // 16-byte vectors a thread is sized for: an entry gets ceil(vectors / (256 * 8)) blocks ...
#define FORK_MAX_BLOCKS 512               // ... at most this many (the rest is the grid stride: 2 blocks of 4 waves per CU)
enum { FORK_FIXED = 0, FORK_ROWS = 1, FORK_BITS = 2 };

struct ForkEntry {
    unsigned char *dst;
    const unsigned char *src;
    unsigned long long bytes;             // the buffer's size (both handles have the same shape)
    int kind, first_block, blocks;
};
struct ForkTable {
    ForkEntry e[FORK_MAX_ENTRIES];
    int n;
};

// (k_stream_fork clears n_work and n_bind as one range of words)
static_assert(offsetof(Counters, n_bind) == offsetof(Counters, n_work) + sizeof(Counters::n_work), "n_bind follows n_work in the counter block");
static_assert(sizeof(Counters) / 4 <= FORK_THREADS && sizeof(Counters) % 4 == 0, "one thread of the first block per word of the counter block");

static inline int fork_blocks(unsigned long long bytes) {
    const unsigned long long per_block = (unsigned long long)FORK_THREADS * FORK_VECS_PER_THREAD * 16;
    return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((bytes + per_block - 1) / per_block, FORK_MAX_BLOCKS));
}

__global__ __launch_bounds__(FORK_THREADS) void k_stream_fork(ForkTable t, Counters *__restrict__ dst_ctr, const Counters *__restrict__ src_ctr) {
    const int b = (int)blockIdx.x;
    if (b == 0 && threadIdx.x < sizeof(Counters) / 4) {
        const uint32_t w = threadIdx.x;
        const uint32_t lo = offsetof(Counters, n_work) / 4, hi = (offsetof(Counters, n_bind) + sizeof(src_ctr->n_bind)) / 4;     // (n_work, n_bind: adjacent)
        const bool clear = (w >= lo && w < hi) || w == offsetof(Counters, error) / 4;
        reinterpret_cast<uint32_t *>(dst_ctr)[w] = clear ? 0u : reinterpret_cast<const uint32_t *>(src_ctr)[w];
    }
    int i = 0;
    while (i + 1 < t.n && b >= t.e[i + 1].first_block) ++i;
    const ForkEntry e = t.e[i];
    // bytes [0, copy) come from the source, bytes [copy, end) are zeroed
    const long long S = max(src_ctr->S, 0);
    unsigned long long copy = e.bytes, end = e.bytes;
    if (e.kind == FORK_ROWS) copy = end = min(e.bytes, (unsigned long long)S * 4);
    else if (e.kind == FORK_BITS) copy = min(e.bytes, (unsigned long long)((S + 31) >> 5) * 4);
    const unsigned long long nvec = end >> 4, cvec = copy >> 4;      // whole vectors in all; whole vectors that are copies
    const uint4 *__restrict__ s4 = reinterpret_cast<const uint4 *>(e.src);
    uint4 *__restrict__ d4 = reinterpret_cast<uint4 *>(e.dst);
    const unsigned long long stride = (unsigned long long)e.blocks * FORK_THREADS;
    for (unsigned long long v = (unsigned long long)(b - e.first_block) * FORK_THREADS + threadIdx.x; v < nvec; v += stride) {
        if (v < cvec) d4[v] = s4[v];
        else if ((v << 4) >= copy) d4[v] = make_uint4(0u, 0u, 0u, 0u);
        else                                                          // (the one vector the boundary cuts: copy is a multiple of 4)
            for (unsigned long long o = v << 4; o < (v << 4) + 16; ++o) e.dst[o] = o < copy ? e.src[o] : (unsigned char)0;
    }
    if (b == e.first_block) {
        const unsigned long long o = (nvec << 4) + threadIdx.x;
        if (o < end) e.dst[o] = o < copy ? e.src[o] : (unsigned char)0;
    }
}

// n consecutive rows of a bank, from row first_row with wrap, into a contiguous buffer: a block per row, 16-byte vectors (rows
// are W = 4 W4 words, the bank and the destination 16-byte aligned)
__global__ __launch_bounds__(256) void k_bank_rows(const uint32_t *__restrict__ bank, int bank_rows, int first_row, int W4, uint32_t *__restrict__ dst) {
    const size_t r = blockIdx.x;
    const size_t row = (size_t)(((long long)first_row + (long long)r) % bank_rows);
    const uint4 *s = reinterpret_cast<const uint4 *>(bank) + row * (size_t)W4;
    uint4 *o = reinterpret_cast<uint4 *>(dst) + r * (size_t)W4;
    for (int w = (int)threadIdx.x; w < W4; w += 256) o[w] = s[w];
}

#endif
