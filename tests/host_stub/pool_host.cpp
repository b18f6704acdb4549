// The host code of htm_pool_columns under AddressSanitizer + UBSan, as a stand-alone program (tests/test_pooling_cpu.py), built and
// linked as tests/host_stub/coordinate_host.cpp is: htm_engine.hip host-only and this file with -fsanitize=address,undefined,
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory, kernels do nothing).  The program is run
// directly; nothing is preloaded.  It drives the entry with exactly-sized heap buffers -- one call, a scratch of one window (a
// batch per window), strides 1 and 5, the largest parameters, a bank that wraps, no reset bits -- and with every refusal, each of
// which must leave the handle usable and launch nothing (the stub counts the launches).  Prints "ok"; exit status 0 on success.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

static htm_handle *make_handle(int input_dim, int enable_sp) {
    htm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_bytes = sizeof(cfg);
    cfg.input_dim = input_dim;
    cfg.column_dim = C;
    cfg.cell_dim = K;
    cfg.active_columns = ACTIVE;
    cfg.enable_sp = enable_sp;
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
    cfg.seed = 3;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static void *dev(size_t bytes) {
    void *p = nullptr;                          // ("device" memory is the host heap in the stub: exactly sized, 16-byte aligned)
    CHECK(posix_memalign(&p, 16, bytes) == 0 && p);
    memset(p, 0, bytes);
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

int main() {
    htm_handle *h = make_handle(LOWER, 1);
    htm_info info;
    CHECK(htm_get_info(h, &info) == HTM_OK);
    const int W = info.words_per_row, PW = (LOWER + 31) / 32;
    CHECK(W == (LOWER + 127) / 128 * 4);
    const int stride = 5, n_rows = 7, bank_rows = 9;
    const size_t window = (size_t)(stride + 8) * 4 * W;
    int32_t *lists = (int32_t *)dev((size_t)n_rows * stride * LISTS_K * 4);
    uint32_t *colpred = (uint32_t *)dev((size_t)n_rows * stride * PW * 4);
    uint8_t *persistence = (uint8_t *)dev(LOWER);
    uint32_t *prev = (uint32_t *)dev((size_t)PW * 4);
    uint32_t *bits = (uint32_t *)dev(4);
    uint32_t *bank = (uint32_t *)dev((size_t)bank_rows * W * 4);
    void *scratch = dev(window * n_rows);
    void *one = dev(window);

    long before = bithtm_stub_kernel_launches();
    const htm_pool_link link = make_link(stride, 1, 8, 1, 16, 40);
    // one batch: three launches
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, (int64_t)(window * n_rows), bank, bank_rows, 4) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before + 3);
    // a scratch of one window: a batch per window
    before = bithtm_stub_kernel_launches();
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, nullptr, one, (int64_t)window, bank, bank_rows, 8) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before + 3 * n_rows);
    // a scratch of two windows and a byte less than a third: four batches
    before = bithtm_stub_kernel_launches();
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, (int64_t)(3 * window - 1), bank, bank_rows, 0) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before + 3 * 4);
    // stride 1 over the same buffers (35 windows would need more bank rows than 9: they wrap), the largest parameters
    before = bithtm_stub_kernel_launches();
    CHECK(htm_pool_columns(h, make_link(1, 255, 255, 255, 255, LOWER), lists, LISTS_K, colpred, n_rows * stride, persistence, prev, bits, scratch,
                           (int64_t)(window * n_rows), bank, bank_rows, 0) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() > before);
    CHECK(htm_pool_columns(h, make_link(1, 0, 1, 1, 1, 1), lists, LISTS_K, colpred, 1, persistence, prev, nullptr, one, (int64_t)window, bank, 1, 0) == HTM_OK);
    // no rows: nothing
    before = bithtm_stub_kernel_launches();
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, 0, persistence, prev, bits, scratch, (int64_t)window, bank, bank_rows, 0) == HTM_OK);
    CHECK(bithtm_stub_kernel_launches() == before);

    // the refusals: nothing launched, the handle goes on
    htm_handle *no_sp = make_handle(LOWER, 0);
    htm_pool_link bad_size = link;
    bad_size.struct_bytes -= 4;
    const int64_t sb = (int64_t)(window * n_rows);
    before = bithtm_stub_kernel_launches();
    CHECK(htm_pool_columns(nullptr, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, nullptr, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, nullptr, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, nullptr, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, nullptr, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, nullptr, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, nullptr, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, bad_size, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, 0, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, -1, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, 0, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, bank_rows) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, -1) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank + 1, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence + 4, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev + 1, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, (char *)scratch + 8, sb, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, (int64_t)window - 1, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, -1, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, INT64_MIN, bank, bank_rows, 0) == HTM_ERR_ARGUMENT);
    const int limits[][6] = {{0, 1, 8, 1, 16, 40}, {-1, 1, 8, 1, 16, 40}, {5, -1, 8, 1, 16, 40}, {5, 256, 8, 1, 16, 40}, {5, 1, -1, 1, 16, 40}, {5, 1, 256, 1, 16, 40},
                             {5, 0, 0, 1, 16, 40}, {5, 1, 8, 0, 16, 40}, {5, 1, 8, 256, 16, 40}, {5, 1, 8, 1, 0, 40}, {5, 1, 8, 1, 256, 40}, {5, 1, 8, 1, 16, 0},
                             {5, 1, 8, 1, 16, LOWER + 1}, {5, 1, 8, 1, 16, -3}, {INT32_MAX, 1, 8, 1, 16, 40}};
    for (const auto &p : limits)
        CHECK(htm_pool_columns(h, make_link(p[0], p[1], p[2], p[3], p[4], p[5]), lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank,
                               bank_rows, 0) == HTM_ERR_ARGUMENT);
    CHECK(htm_pool_columns(no_sp, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_ERR_STATE);
    CHECK(bithtm_stub_kernel_launches() == before);
    CHECK(strstr(htm_last_error(no_sp), "htm_pool_columns") != nullptr);
    CHECK(htm_pool_columns(h, link, lists, LISTS_K, colpred, n_rows, persistence, prev, bits, scratch, sb, bank, bank_rows, 0) == HTM_OK);
    CHECK(htm_sync(h) == HTM_OK);

    htm_destroy(no_sp);
    htm_destroy(h);
    void *all[] = {lists, colpred, persistence, prev, bits, bank, scratch, one};
    for (void *p : all) free(p);
    printf("ok\n");
    return 0;
}
