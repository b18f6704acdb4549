// The host code of htm_group_pack_columns and htm_group_pool_columns under AddressSanitizer + UBSan, as a stand-alone program
// (tests/test_group_stack_cpu.py), built and linked as tests/host_stub/pool_host.cpp is: htm_engine.hip host-only and this file
// with -fsanitize=address,undefined, against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory, kernels do
// nothing).  The program is run directly; nothing is preloaded.  It drives both entries over groups of 1, 3 and 7 members with
// exactly-sized heap buffers -- the launches of every call against a twin of the batching arithmetic, the group's table growing
// from a pack call's to a pooled call's and reused after that (every copy into it is checked by the sanitizer), reset bits for some
// members only -- and every refusal, each of which must leave the group usable and launch nothing.  Prints "ok"; exit status 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"

extern "C" long bithtm_stub_kernel_launches(void);

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int LOWER = 1000, C = 64, K = 4, ACTIVE = 4, LISTS_K = 20;

static htm_handle *make_handle(int seed, void *stream) {
    htm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_bytes = sizeof(cfg);
    cfg.input_dim = LOWER;
    cfg.column_dim = C;
    cfg.cell_dim = K;
    cfg.active_columns = ACTIVE;
    cfg.enable_sp = 1;
    cfg.enable_tm = 1;
    cfg.sp_permanence_threshold = 0.0;
    cfg.sp_delta_on = 0.1;
    cfg.sp_delta_off = -0.02;
    cfg.boost_coefficient = -50.0f;
    cfg.duty_momentum = 0.99f;
    cfg.duty_increment = 0.01f;
    cfg.tm_learn_active = 0.1;
    cfg.tm_learn_inactive = -0.1;
    cfg.tm_punish_active = -0.01;
    cfg.tm_punish_inactive = 0.0;
    cfg.tm_learn_prune = 1;
    cfg.tm_punish_prune = 1;
    cfg.tm_permanence_initial = 0.21f;
    cfg.tm_permanence_threshold = 0.5f;
    cfg.segment_activation_threshold = 10;
    cfg.segment_matching_threshold = 8;
    cfg.segment_sampling_synapses = 32;
    cfg.segment_capacity = 1024;
    cfg.segment_slots = 64;
    cfg.seed = seed;
    cfg.use_caller_stream = stream != nullptr;
    cfg.stream = stream;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static std::vector<void *> g_all;
static void *dev(size_t bytes) {
    void *p = nullptr;                          // ("device" memory is the host heap in the stub: exactly sized, 16-byte aligned)
    CHECK(posix_memalign(&p, 16, bytes) == 0 && p);
    memset(p, 0, bytes);
    g_all.push_back(p);
    return p;
}

static htm_pool_link make_link(int stride, int aw, int pw, int decay, int ceiling, int union_bits) {
    htm_pool_link l;
    memset(&l, 0, sizeof(l));
    l.struct_bytes = sizeof(l);
    l.stride = stride;
    l.active_weight = aw;
    l.predicted_weight = pw;
    l.decay = decay;
    l.ceiling = ceiling;
    l.union_bits = union_bits;
    return l;
}

// the twin of the entry's batching: launches of a pooled call of n_rows windows over B members with scratch_bytes of scratch
static long twin_launches(int64_t scratch_bytes, int B, int stride, int W, int n_rows) {
    if (n_rows == 0) return 0;
    const int64_t window = (int64_t)(stride + 8) * 4 * W;
    int64_t per_batch = scratch_bytes / (B * window);
    if (per_batch > n_rows) per_batch = n_rows;
    return 3 * ((n_rows + per_batch - 1) / per_batch);
}

static void drive(int B) {
    // the group's members on ONE stream (the first member's own: htm_get_stream hands it out)
    std::vector<htm_handle *> members;
    members.push_back(make_handle(1, nullptr));
    void *stream = nullptr;
    CHECK(htm_get_stream(members[0], &stream) == HTM_OK);
    for (int i = 1; i < B; ++i) members.push_back(make_handle(1 + i, stream));
    htm_group *g = nullptr;
    CHECK(htm_group_create(members.data(), B, &g) == HTM_OK && g);
    htm_info info;
    CHECK(htm_get_info(members[0], &info) == HTM_OK);
    const int W = info.words_per_row, PW = (LOWER + 31) / 32;
    const int stride = 5, n_rows = 7, bank_rows = 9;
    const size_t window = (size_t)(stride + 8) * 4 * W;
    std::vector<const int32_t *> lists(B);
    std::vector<const uint32_t *> colpred(B), bits(B);
    std::vector<uint8_t *> persistence(B);
    std::vector<uint32_t *> prev(B), banks(B);
    std::vector<int32_t> first(B);
    for (int i = 0; i < B; ++i) {
        lists[i] = (const int32_t *)dev((size_t)n_rows * stride * LISTS_K * 4);
        colpred[i] = (const uint32_t *)dev((size_t)n_rows * stride * PW * 4);
        persistence[i] = (uint8_t *)dev(LOWER);
        prev[i] = (uint32_t *)dev((size_t)PW * 4);
        bits[i] = i % 2 ? nullptr : (const uint32_t *)dev(4);          // reset bits for every other member
        banks[i] = (uint32_t *)dev((size_t)bank_rows * W * 4);
        first[i] = (3 * i + 8) % bank_rows;
    }
    const size_t whole = window * n_rows * B;
    void *scratch = dev(whole);
    const htm_pool_link link = make_link(stride, 1, 8, 1, 16, 40);

    // pack: one launch whatever B is (the group's table is made for B pack rows here ...)
    long before = bithtm_stub_kernel_launches();
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before + 1);
    // (... grows for the pooled call, and serves the pack call after it as it is)
    const int64_t scratches[] = {(int64_t)whole, (int64_t)(window * B), (int64_t)(3 * window * B - 1), (int64_t)(window * B * 2), (int64_t)whole * 4};
    for (int64_t sb : scratches) {
        before = bithtm_stub_kernel_launches();
        // (a scratch larger than the buffer is never touched beyond the batches' parts: per_batch <= n_rows)
        CHECK(htm_group_pool_columns(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(),
                                     bank_rows, first.data()) == HTM_OK);
        CHECK(bithtm_stub_kernel_launches() == before + twin_launches(sb, B, stride, W, n_rows));
    }
    CHECK(twin_launches((int64_t)(window * B), B, stride, W, n_rows) == 3 * n_rows && twin_launches((int64_t)whole, B, stride, W, n_rows) == 3);
    before = bithtm_stub_kernel_launches();
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows * stride, 1, banks.data(), bank_rows, first.data()) == HTM_OK);       // (35 rows wrap a bank of 9)
    CHECK(htm_group_pool_columns(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), nullptr, scratch, (int64_t)whole,
                                 banks.data(), bank_rows, first.data()) == HTM_OK);                                                   // no reset bits at all
    CHECK(htm_group_pool_columns(g, make_link(1, 255, 255, 255, 255, LOWER), lists.data(), LISTS_K, colpred.data(), n_rows * stride, persistence.data(), prev.data(),
                                 bits.data(), scratch, (int64_t)whole, banks.data(), bank_rows, first.data()) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() > before + 4);
    before = bithtm_stub_kernel_launches();
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, 0, stride, banks.data(), bank_rows, first.data()) == HTM_OK);
    CHECK(htm_group_pool_columns(g, link, lists.data(), LISTS_K, colpred.data(), 0, persistence.data(), prev.data(), bits.data(), scratch, (int64_t)whole, banks.data(),
                                 bank_rows, first.data()) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before);

    // the refusals: nothing launched, the group goes on
    const int64_t sb = (int64_t)whole;
    const int last = B - 1;
    before = bithtm_stub_kernel_launches();
#define POOL(...) htm_group_pool_columns(__VA_ARGS__)
#define ARGS_OK lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()
    CHECK(POOL(nullptr, link, ARGS_OK) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, nullptr, LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, nullptr, n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, nullptr, prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), nullptr, bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), nullptr, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, nullptr, bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, nullptr) == HTM_ERR_ARGUMENT);
    {   // a hole, a misaligned address or a bad first row in the LAST member's entry of each array
        auto l2 = lists; l2[last] = nullptr;
        CHECK(POOL(g, link, l2.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        auto c2 = colpred; c2[last] = nullptr;
        CHECK(POOL(g, link, lists.data(), LISTS_K, c2.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        auto p2 = persistence; p2[last] = nullptr;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, p2.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        p2[last] = persistence[last] + 4;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, p2.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        auto v2 = prev; v2[last] = nullptr;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), v2.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        v2[last] = prev[last] + 1;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), v2.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        auto b2 = banks; b2[last] = nullptr;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, b2.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, b2.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_group_pack_columns(g, l2.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        b2[last] = banks[last] + 1;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, b2.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, b2.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
        for (int32_t row : {-1, bank_rows, INT32_MAX, INT32_MIN}) {
            auto f2 = first; f2[last] = row;
            CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, f2.data()) == HTM_ERR_ARGUMENT);
            CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, f2.data()) == HTM_ERR_ARGUMENT);
        }
    }
    htm_pool_link bad_size = link;
    bad_size.struct_bytes -= 4;
    CHECK(POOL(g, bad_size, ARGS_OK) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), 0, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), -1, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, sb, banks.data(), 0, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), (char *)scratch + 8, sb, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    // a scratch of one window for all members but one byte; negative sizes
    for (int64_t small : {(int64_t)(window * B) - 1, (int64_t)window, (int64_t)0, (int64_t)-1, INT64_MIN}) {
        if (small == (int64_t)window && B == 1) continue;
        CHECK(POOL(g, link, lists.data(), LISTS_K, colpred.data(), n_rows, persistence.data(), prev.data(), bits.data(), scratch, small, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    }
    const int limits[][6] = {{0, 1, 8, 1, 16, 40}, {-1, 1, 8, 1, 16, 40}, {5, -1, 8, 1, 16, 40}, {5, 256, 8, 1, 16, 40}, {5, 1, -1, 1, 16, 40}, {5, 1, 256, 1, 16, 40},
                             {5, 0, 0, 1, 16, 40}, {5, 1, 8, 0, 16, 40}, {5, 1, 8, 256, 16, 40}, {5, 1, 8, 1, 0, 40}, {5, 1, 8, 1, 256, 40}, {5, 1, 8, 1, 16, 0},
                             {5, 1, 8, 1, 16, LOWER + 1}, {5, 1, 8, 1, 16, -3}, {INT32_MAX, 1, 8, 1, 16, 40}};
    for (const auto &p : limits) CHECK(POOL(g, make_link(p[0], p[1], p[2], p[3], p[4], p[5]), ARGS_OK) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(nullptr, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, nullptr, LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, nullptr, bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), 0, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, -1, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, 0, banks.data(), bank_rows, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, banks.data(), 0, first.data()) == HTM_ERR_ARGUMENT);
    CHECK(bithtm_stub_kernel_launches() == before);
    CHECK(strstr(htm_group_last_error(g), "htm_group_pack_columns") != nullptr);

    // a group with a member on a stream of its own: HTM_ERR_STATE from both entries, nothing launched
    if (B > 1) {
        std::vector<htm_handle *> mixed(members.begin(), members.end());
        htm_handle *alone = make_handle(99, nullptr);
        mixed[last] = alone;
        htm_group *gm = nullptr;
        CHECK(htm_group_create(mixed.data(), B, &gm) == HTM_OK && gm);
        before = bithtm_stub_kernel_launches();
        CHECK(POOL(gm, link, ARGS_OK) == HTM_ERR_STATE && strstr(htm_group_last_error(gm), "another stream"));
        CHECK(htm_group_pack_columns(gm, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_ERR_STATE);
        CHECK(bithtm_stub_kernel_launches() == before);
        htm_group_destroy(gm);
        htm_destroy(alone);
    }
    before = bithtm_stub_kernel_launches();
    CHECK(POOL(g, link, ARGS_OK) == HTM_OK);
    CHECK(htm_group_pack_columns(g, lists.data(), LISTS_K, n_rows, stride, banks.data(), bank_rows, first.data()) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before + 4);
    CHECK(htm_sync(members[0]) == HTM_OK);
    htm_group_destroy(g);
    for (htm_handle *h : members) htm_destroy(h);
}

int main() {
    for (int B : {1, 3, 7}) drive(B);
    for (void *p : g_all) free(p);
    printf("ok\n");
    return 0;
}
