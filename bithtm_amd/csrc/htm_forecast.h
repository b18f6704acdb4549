// Closed-loop forecasting (htm_encode_votes, htm_set_run_feedback; include/bithtm_hip.h): the link between
// a state's predicted-input votes (htm_decode.h) and the bank row the next step reads.
//
//   row = encode(votes, min_votes, max_bits):  x[i] = votes[i] >= min_votes; if max_bits > 0 and more than max_bits inputs pass,
//   only the max_bits with the most votes stay, ties at the cut-off going to the LOWER input index.
//
// One block encodes one row (W words = input_dim padded to 128 bits, pad bits 0, every word written: no memset, as
// k_pack_columns).  The row is cut into one contiguous run of 64-input chunks per wave, so that a wave walks its inputs in index
// order with coalesced loads (64 consecutive int32 per load), and a ballot over a chunk is the chunk's two output words.
//   threshold form (max_bits == 0, or no more than max_bits candidates): one pass -- load, ballot, one 8-byte store per chunk.
//   capped form: (a) a pass counts the candidates and finds the largest vote; (b) a radix select over the candidates' votes, 12
//     bits per pass from the top bit of the largest vote down (one pass unless a vote reaches 4 096), each pass a 4 096-bin LDS
//     histogram and a block scan from the top bin, finds the cut-off v* = the max_bits-th largest vote and the quota of inputs
//     AT v* that still fit; (c) every wave counts the ties at v* in its run, the counts of the waves before it are its offset;
//     (d) the output pass admits votes above v*, and a tie while offset + (ties before it in the chunk: ballot, prefix popcount)
//     is below the quota.
// The votes row is read three or four times in the capped form; it is at most a few hundred KB and stays in L2.
// The votes are a scratch row that role_pin adds into (htm_decode.h): the output pass leaves it zeroed for the next use.
#ifndef BITHTM_HTM_FORECAST_H
#define BITHTM_HTM_FORECAST_H

#define ENC_THREADS 256
#define ENC_WAVES (ENC_THREADS / 64)
#define ENC_DIGIT 12
#define ENC_BINS (1 << ENC_DIGIT)

// device-side descriptor of a handle's run feedback (filled by htm_set_run_feedback; graphs of feeding steps hold its address)
struct FeedDev {
    uint32_t *bank;            // the bank the feeding runs read and write, or null: no feedback
    int32_t *votes;            // the handle's scratch votes row [I], zero between uses
    int32_t n_inputs;          // rows of the bank
    int32_t min_votes, max_bits;
};

__global__ void k_feed_set(FeedDev *r, uint32_t *bank, int32_t *votes, int32_t n_inputs, int32_t min_votes, int32_t max_bits) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        r->bank = bank;
        r->votes = votes;
        r->n_inputs = n_inputs;
        r->min_votes = min_votes;
        r->max_bits = max_bits;
    }
}

// votes[0, I) -> row[0, W); all ENC_THREADS threads of the block call, with the same arguments
__device__ __forceinline__ void role_encode(int32_t *__restrict__ votes, int I, int W, int min_votes, int max_bits, uint32_t *__restrict__ row) {
    __shared__ uint32_t s_hist[ENC_BINS];
    __shared__ uint32_t s_wave[ENC_WAVES];
    __shared__ int s_cand, s_max;
    __shared__ uint32_t s_prefix, s_need;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const int n_chunks = W >> 1;                      // 64 inputs = two words each (W is a multiple of 4)
    const int per_wave = (n_chunks + ENC_WAVES - 1) / ENC_WAVES;
    const int c0 = min(wave * per_wave, n_chunks), c1 = min(c0 + per_wave, n_chunks);
    // what the output pass admits: votes above vstar, and the first `quota` inputs (in index order) AT vstar
    int vstar = min_votes - 1;
    uint32_t quota = 0;
    if (max_bits > 0) {
        if (threadIdx.x == 0) { s_cand = 0; s_max = 0; }
        __syncthreads();
        int cand = 0, vmax = 0;
        for (int c = c0; c < c1; ++c) {
            const int i = c * 64 + lane;
            const int v = i < I ? votes[i] : 0;
            cand += __popcll(__ballot(v >= min_votes));
            vmax = max(vmax, v);
        }
        vmax = (int)wave_reduce64((u64)(uint32_t)vmax, 0ull, [](u64 a, u64 b) { return a > b ? a : b; });
        if (lane == 0) { atomicAdd(&s_cand, cand); atomicMax(&s_max, vmax); }
        __syncthreads();
        if (s_cand > max_bits) {                      // (the same answer in every thread of the block)
            const int top = 32 - __clz(s_max);        // bits of the largest vote (>= 1: it is a candidate, min_votes >= 1)
            uint32_t prefix = 0, need = (uint32_t)max_bits;
            for (int shift = ((top - 1) / ENC_DIGIT) * ENC_DIGIT; shift >= 0; shift -= ENC_DIGIT) {
                for (int b = (int)threadIdx.x; b < ENC_BINS; b += ENC_THREADS) s_hist[b] = 0;
                __syncthreads();
                for (int c = c0; c < c1; ++c) {
                    const int i = c * 64 + lane;
                    const int v = i < I ? votes[i] : 0;
                    const bool in = v >= min_votes && (uint32_t)((u64)(uint32_t)v >> (shift + ENC_DIGIT)) == prefix;
                    hist_add_tie(s_hist, ((uint32_t)v >> shift) & (ENC_BINS - 1), in);
                }
                __syncthreads();
                // thread t owns the bins [ENC_BINS - 16 (t + 1), ENC_BINS - 16 t): an exclusive scan over the threads counts from the top bin
                const int hi = ENC_BINS - (ENC_BINS / ENC_THREADS) * (int)threadIdx.x;
                uint32_t mine = 0;
#pragma unroll
                for (int j = 1; j <= ENC_BINS / ENC_THREADS; ++j) mine += s_hist[hi - j];
                uint32_t total;
                uint32_t above = block_excl_scan<ENC_THREADS>(mine, s_wave, total);
                if (above < need && need <= above + mine) {       // (one thread: the bin of the need-th largest)
                    for (int j = 1; j <= ENC_BINS / ENC_THREADS; ++j) {
                        const uint32_t n = s_hist[hi - j];
                        if (need <= above + n) { s_prefix = (prefix << ENC_DIGIT) | (uint32_t)(hi - j); s_need = need - above; break; }
                        above += n;
                    }
                }
                __syncthreads();
                prefix = s_prefix;
                need = s_need;
            }
            vstar = (int)prefix;
            quota = need;
        }
    }
    uint32_t offset = 0;                              // ties at vstar in the runs of the waves before this one
    if (quota) {
        uint32_t ties = 0;
        for (int c = c0; c < c1; ++c) {
            const int i = c * 64 + lane;
            ties += (uint32_t)__popcll(__ballot(i < I && votes[i] == vstar));
        }
        if (lane == 0) s_wave[wave] = ties;
        __syncthreads();
        for (int w = 0; w < wave; ++w) offset += s_wave[w];
    }
    for (int c = c0; c < c1; ++c) {
        const int i = c * 64 + lane;
        const int v = i < I ? votes[i] : 0;
        const bool tie = quota && i < I && v == vstar;
        const u64 tb = __ballot(tie);
        const bool admit = v > vstar || (tie && offset + (uint32_t)__popcll(tb & lanemask_lt()) < quota);
        offset += (uint32_t)__popcll(tb);
        const u64 m = __ballot(admit);
        if (lane == 0) *reinterpret_cast<uint2 *>(row + 2 * (size_t)c) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));   // (rows are 16-byte aligned)
        if (i < I) votes[i] = 0;
    }
}

// htm_encode_votes: the handle's scratch votes (k_pin has just added the current state's into them) into one bank row
__global__ __launch_bounds__(ENC_THREADS) void k_encode(Dev d, int32_t *votes, int min_votes, int max_bits, uint32_t *row) {
    role_encode(votes, d.I, d.W, min_votes, max_bits, row);
}

// Behind step p's last launch in a feeding run: the votes of the state the step leaves (k_feed_votes), then bank row
// (step index + 1) % n_inputs, the row the next step's overlap reads (k_feed_step)
__global__ __launch_bounds__(256) void k_feed_votes(Dev d, int p, const FeedDev *r) { role_pin(d, p, r->votes); }

__global__ __launch_bounds__(ENC_THREADS) void k_feed_step(Dev d, int p, const FeedDev *r) {
    const size_t slot = (d.ctr->step[p] + 1u) % (uint32_t)r->n_inputs;
    role_encode(r->votes, d.I, d.W, r->min_votes, r->max_bits, r->bank + slot * (size_t)d.W);
}

// model groups (htm_group.h): grid y = member, each member's own descriptor; a member without feedback (null bank) does nothing
__global__ __launch_bounds__(256) void kgrp_feed_votes(const Dev *__restrict__ tab, int p, FeedDev *const *__restrict__ feeds) {
    const FeedDev *r = feeds[blockIdx.y];
    if (!r->bank) return;
    role_pin(tab[blockIdx.y], p, r->votes);
}

__global__ __launch_bounds__(ENC_THREADS) void kgrp_feed_step(const Dev *__restrict__ tab, int p, FeedDev *const *__restrict__ feeds) {
    const Dev &d = tab[blockIdx.y];
    const FeedDev *r = feeds[blockIdx.y];
    if (!r->bank) return;
    const size_t slot = (d.ctr->step[p] + 1u) % (uint32_t)r->n_inputs;
    role_encode(r->votes, d.I, d.W, r->min_votes, r->max_bits, r->bank + slot * (size_t)d.W);
}

#endif
