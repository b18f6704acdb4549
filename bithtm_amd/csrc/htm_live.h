// Live ticks of a model group (htm_live_tick, htm_live_reset; include/bithtm_hip.h): one call per tick of B
// streams -- values or packed rows in, every member's counters, capacity flags and decoded predictions out -- whose copies,
// launches and waits do not depend on B.  Around the step launches of htm_group.h the tick enqueues at most three launches:
//   klive_reset   before the record's begin launch: the sequence reset of k_tm_reset (role_tm_reset, htm_reset.h) for the members
//                 whose staged flag is set; grid y = member, and a block of an unflagged member returns at once
//   k_bank_encode (htm_scalar.h, as it is) over the B value rows: member i's row of the group's staging bank
//   klive_finish  behind the step's record and votes launches: per member and field the decode of k_decode_votes
//                 (role_decode_votes, htm_scalar.h) over the member's vote row, and per member the result row
// Part of the single translation unit htm_engine.hip (included after htm_group.h).
#ifndef BITHTM_HTM_LIVE_H
#define BITHTM_HTM_LIVE_H

// a member's staged reset flag: bit 0 = reset before the coming step, bit 1 = that step's parity (the member's own: htm_live_reset
// takes members of either parity)
#define LIVE_RESET 1
#define LIVE_PARITY 2

// grid (reset_blocks, B).  The coming step's index is the one the last completed step left in the member's counter block, as
// kgrp_rec_begin reads it.  The gate is block-uniform; every loop of the role is bounded by the member's own shape and its own
// Counters::S.  Nothing is recorded here: the tick's record begins behind this launch and counts the cleared prediction words.
__global__ __launch_bounds__(256) void klive_reset(const Dev *__restrict__ tab, const int32_t *__restrict__ flags) {
    const int f = flags[blockIdx.y];
    if (!(f & LIVE_RESET)) return;
    const Dev &d = tab[blockIdx.y];
    const int p = (f & LIVE_PARITY) ? 1 : 0;
    role_tm_reset(d, p, nullptr, d.ctr->step[p]);
}

// grid (max(n_fields, 1), B), behind step p's record and votes launches.  Block (j, i): field j of member i's vote row decoded into
// pairs[i][j] = (bucket, score); block (0, i) also fills member i's result row -- its record slot, the index of the step just
// taken and the sticky capacity flags -- with plain vector stores.
__global__ __launch_bounds__(SCALAR_THREADS) void klive_finish(const Dev *__restrict__ tab, int p, ScalarTab ftab, int n_fields,
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
        role_decode_votes(ftab.f[blockIdx.x], votes + (size_t)i * (size_t)d.I, pairs + ((size_t)i * n_fields + blockIdx.x) * 2);
}

#endif
