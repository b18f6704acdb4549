// The statements of a select block of pooling links over the descriptor `a` (a PoolDev in scope), written once and included as
// text by kpool_select (htm_pool.h) and its member-indexed twin kgpool_select (htm_group_stack.h).  Text, not a __device__ function:
// inlined from a function the same statements get another instruction order from the compiler and kpool_select seven more VGPRs
// than it had (38 for 31; the scan's and the pack's bodies are functions and compile to what they were).
    extern __shared__ __attribute__((aligned(16))) uint32_t s_row[];            // [W]
    __shared__ uint32_t s_hist[POOL_WAVES][256], s_scan[POOL_WAVES], s_sel[4];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const size_t r = blockIdx.x;
    const int n16 = a.W * 2;                                                    // 16-byte pieces of the snapshot row = 16-bit pieces of the bitmap
    const uint4 *row4 = reinterpret_cast<const uint4 *>(a.snap + r * (size_t)a.W * 32);
    for (int i = tid; i < POOL_WAVES * 256; i += POOL_THREADS) (&s_hist[0][0])[i] = 0u;
    __syncthreads();
    for (int q = tid; q < n16; q += POOL_THREADS) {
        const uint4 v = row4[q];
        if ((v.x | v.y | v.z | v.w) == 0u) continue;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const uint32_t b = (w[u >> 2] >> (8 * (u & 3))) & 255u;
            if (b) atomicAdd(&s_hist[wave][b], 1u);
        }
    }
    __syncthreads();
    // thread t looks at the value 255 - t: `incl` columns have that value or a larger one (the value 0 is never counted)
    uint32_t mine = 0u;
#pragma unroll
    for (int u = 0; u < POOL_WAVES; ++u) mine += s_hist[u][255 - tid];
    const uint32_t scan = wave_incl_scan(mine);
    if (lane == 63) s_scan[wave] = scan;
    __syncthreads();
    uint32_t incl = scan;
#pragma unroll
    for (int u = 0; u < POOL_WAVES; ++u) incl += u < wave ? s_scan[u] : 0u;
    if (tid == POOL_THREADS - 1) s_sel[3] = incl;                               // the columns with P > 0
    __syncthreads();
    const uint32_t take = min((uint32_t)a.union_bits, s_sel[3]);
    if (take == 0u) {
        if (tid == 0) {
            s_sel[0] = 256u;                                                    // a cut no byte reaches: an empty row
            s_sel[1] = 0u;
            s_sel[2] = 0u;
        }
    } else if (incl - mine < take && take <= incl) {                            // (exactly one thread, and mine >= 1)
        s_sel[0] = (uint32_t)(255 - tid);
        s_sel[1] = take - (incl - mine);
        s_sel[2] = mine;
    }
    __syncthreads();
    const uint32_t cut = s_sel[0], want = s_sel[1], ties = s_sel[2];
    uint16_t *s_row16 = reinterpret_cast<uint16_t *>(s_row);
    uint32_t seen = 0u;                                                         // columns at the cut below this trip's
    for (int q0 = 0; q0 < n16; q0 += POOL_THREADS) {                            // (block-uniform bounds: the barriers inside are met by all)
        const int q = q0 + tid;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q < n16) v = row4[q];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t above = 0u, at = 0u;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const uint32_t b = (w[u >> 2] >> (8 * (u & 3))) & 255u;
            above |= (b > cut ? 1u : 0u) << u;
            at |= (b == cut ? 1u : 0u) << u;
        }
        uint32_t bits = above | at;
        if (want != ties) {                                                     // not every column at the cut wins: the `want` of the lowest index
            const uint32_t n_at = (uint32_t)__popc(at);
            const uint32_t sc = wave_incl_scan(n_at);
            if (lane == 63) s_scan[wave] = sc;
            __syncthreads();
            uint32_t before = seen + sc - n_at, total = 0u;
#pragma unroll
            for (int u = 0; u < POOL_WAVES; ++u) {
                const uint32_t t = s_scan[u];
                before += u < wave ? t : 0u;
                total += t;
            }
            seen += total;
            // the at-cut columns of this thread have the ranks before, before + 1, ...: the first `room` of them win
            const uint32_t room = before < want ? want - before : 0u;
            uint32_t keep = at;
            if (room < n_at) {
                keep = 0u;
                uint32_t left = at;
                for (uint32_t i = 0u; i < room; ++i) {                          // (room < 16)
                    const uint32_t low = left & (0u - left);
                    keep |= low;
                    left ^= low;
                }
            }
            bits = above | keep;
            __syncthreads();                                                    // (s_scan is written again in the next trip)
        }
        if (q < n16) s_row16[q] = (uint16_t)bits;
    }
    __syncthreads();
    const size_t row = (size_t)(((long long)a.first_row + (long long)r) % a.bank_rows);
    uint4 *dst = reinterpret_cast<uint4 *>(a.bank + row * (size_t)a.W);
    const uint4 *s_row4 = reinterpret_cast<const uint4 *>(s_row);
    for (int i = tid; i < (a.W >> 2); i += POOL_THREADS) dst[i] = s_row4[i];
