// Stacks of model groups (htm_group_pack_columns, htm_group_pool_columns; include/bithtm_hip.h): the links
// of B streams' hierarchies in launches whose count does not depend on B.
//
// Every kernel here is a one-stream body of htm_stack.h or htm_pool.h given its member's descriptor: the member is blockIdx.y,
// blockIdx.x is what it is in the solo twin.  The descriptor is read once per block, at an address that is uniform over the block
// (scalar loads); no block waits for another; the rows go out with the bodies' 16-byte stores.
//
//   kgrp_pack_columns  grid (rows, B), dynamic LDS as k_pack_columns: member m's Dev from the group's device table, its lists, bank
//                      and first row from the call's table (GrpPackRow).  `list_offset` -- entries of every member's lists in front
//                      of this launch's first row -- goes by value: the batches of a pooled call share one table.  A bad id sets the
//                      sticky bit 64 in member m's counter block only (the body's d.ctr is the member's).
//   kgpool_scan        grid (ceil(32 W / 256), B): kpool_scan's thread over tab[m] moved to the batch (gpool_member).
//   kgpool_select      grid (windows, B), dynamic LDS as kpool_select: kpool_select's block over tab[m] moved to the batch.
//
// The table of a pooled call holds, per member, the PoolDev of the WHOLE call (first_row, colpred and n_windows of its first window;
// bitmaps and snap: the member's part of the scratch, the same in every batch); the batch -- windows done before it, windows in it --
// goes by value.
#ifndef BITHTM_HTM_GROUP_STACK_H
#define BITHTM_HTM_GROUP_STACK_H

#define GSTACK_MAX_MEMBERS 65535            // grid y

struct GrpPackRow {
    const int32_t *lists;
    uint32_t *bank;
    int32_t first_row, pad;
};

// the scratch of a pooled group call: member m's part is m * gpool_member_bytes(...) bytes in, laid out as the solo call's batch of
// `per_batch` windows (per_batch * stride bitmap rows, then per_batch snapshot rows)
static inline size_t gpool_member_bytes(int W, int stride, int per_batch) { return (size_t)per_batch * pool_window_bytes(W, stride); }

#ifdef __HIPCC__

__global__ __launch_bounds__(PACK_THREADS) void kgrp_pack_columns(const Dev *__restrict__ devs, const GrpPackRow *__restrict__ tab, long long list_offset,
                                                                  int32_t k, int32_t stride, int32_t bank_rows) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_row[];            // [W]
    const GrpPackRow t = tab[blockIdx.y];
    pack_columns_block(devs[blockIdx.y], t.lists + list_offset, k, stride, t.bank, bank_rows, t.first_row, s_row);
}

// member descriptor t of the whole call -> the batch of n windows behind r0 windows
__device__ __forceinline__ PoolDev gpool_member(const PoolDev &t, int r0, int n) {
    PoolDev a = t;
    a.n_windows = n;
    a.first_row = (int)(((long long)t.first_row + (long long)r0) % t.bank_rows);
    a.colpred = t.colpred + (size_t)r0 * (size_t)t.stride * (size_t)t.PW;
    return a;
}

__global__ __launch_bounds__(POOL_THREADS) void kgpool_scan(const PoolDev *__restrict__ tab, int r0, int n) {
    pool_scan_thread(gpool_member(tab[blockIdx.y], r0, n));
}

__global__ __launch_bounds__(POOL_THREADS) void kgpool_select(const PoolDev *__restrict__ tab, int r0, int n) {
    const PoolDev a = gpool_member(tab[blockIdx.y], r0, n);
#include "htm_pool_select.inc"
}

#endif  // __HIPCC__
#endif
