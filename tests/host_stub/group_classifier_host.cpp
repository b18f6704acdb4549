// The host code of the classifier bank under AddressSanitizer + UBSan, as a stand-alone program (tests/test_group_classifier_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked against
// tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on both sides,
// kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_classifiers_create, _update, _reset,
// _read_weights, _write_weights, _state_bytes, _export, _import, htm_set_group_run_active_cells with recorded group runs and
// htm_classifiers_tick through the C ABI, with every refusal (each must leave the objects usable), the one-stream calls on a bank, and
// shared weights destroyed in either order.  With a file name as its argument it then evaluates the member-indexing arithmetic of the
// bank's kernels (bithtm_amd/csrc/htm_classifier.h, compiled here for the host) over the cases of that file and prints every result;
// the test compares them with the definition's layout, computed in Python.
//   y <y> <H>                        -> member, horizon                    (a learning launch's block row)
//   f <y> <H> <n>                    -> member, step, horizon              (a frozen launch's block row)
//   c <streams> <H>                  -> steps per frozen launch
//   r <m> <H> <h>                    -> the row of the [n][H] arrays
//   o <m> <n_steps> <H>              -> the member's first output row
// Exit status 0 and "ok" as the last line on success.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"
#include "../../bithtm_amd/csrc/htm_classifier.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48, WPC = 2;

static htm_handle *make_handle(uint32_t seed, int shard_world = 1, int enable_sp = 1) {
    htm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_bytes = sizeof(cfg);
    cfg.input_dim = enable_sp ? I : 0;
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
    cfg.segment_capacity = 4096;
    cfg.segment_slots = 64;
    cfg.seed = seed;
    cfg.use_caller_stream = 1;                  // (with a NULL stream: the default stream)
    cfg.shard_world = shard_world;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if ((shard_world > 1 || !enable_sp) && rc != HTM_OK) return nullptr;
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static htm_classifier_config config(int buckets, std::vector<int> steps, int alpha_q, int units, int cell_dim, int max_pairs) {
    htm_classifier_config c;
    memset(&c, 0, sizeof(c));
    c.struct_bytes = sizeof(c);
    c.buckets = buckets;
    c.n_steps = (int32_t)steps.size();
    c.alpha_q = alpha_q;
    c.units = units;
    c.cell_dim = cell_dim;
    c.max_pairs = max_pairs;
    for (size_t i = 0; i < steps.size() && i < 8; ++i) c.steps[i] = steps[i];
    return c;
}

static void arithmetic(const char *path) {
    FILE *f = fopen(path, "r");
    CHECK(f);
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        int a, b, c;
        if (kind[0] == 'y') {
            CHECK(fscanf(f, "%d %d", &a, &b) == 2);
            printf("%d %d\n", gcls_member(a, b), gcls_horizon(a, b));
        } else if (kind[0] == 'f') {
            CHECK(fscanf(f, "%d %d %d", &a, &b, &c) == 3);
            printf("%d %d %d\n", gcls_frozen_member(a, b, c), gcls_frozen_step(a, b, c), gcls_horizon(a, b));
        } else if (kind[0] == 'c') {
            CHECK(fscanf(f, "%d %d", &a, &b) == 2);
            printf("%d\n", gcls_chunk(a, b));
        } else if (kind[0] == 'r') {
            CHECK(fscanf(f, "%d %d %d", &a, &b, &c) == 3);
            printf("%" PRId64 "\n", gcls_row(a, b, c));
        } else if (kind[0] == 'o') {
            CHECK(fscanf(f, "%d %d %d", &a, &b, &c) == 3);
            printf("%" PRId64 "\n", gcls_out_row(a, b, c));
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    const int N = 3;
    htm_handle *hs[N] = {make_handle(7), make_handle(8), make_handle(9)};
    htm_handle *h = hs[0];
    std::vector<int32_t> table(HTM_CLASSIFIER_EXP, 1 << 20);    // exactly 2049: one fewer read is the sanitizer's to report
    const int pairs = ACTIVE * WPC;
    const htm_classifier_config small = config(5, {0, 1, 5}, 655, C * K, K, pairs);

    // ---- create: refusals, then objects
    htm_classifier *bank = nullptr, *one = nullptr, *owner = nullptr, *sharer = nullptr, *bad = (htm_classifier *)1;
    CHECK(htm_classifiers_create(nullptr, &small, table.data(), N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_classifiers_create(h, nullptr, table.data(), N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_classifiers_create(h, &small, nullptr, N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_classifiers_create(h, &small, table.data(), N, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_create(h, &small, table.data(), 0, nullptr, &bad) == HTM_ERR_ARGUMENT && !bad);
    CHECK(htm_classifiers_create(h, &small, table.data(), -1, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_classifiers_create(h, &small, table.data(), 65535 / 3 + 1, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank && strstr(htm_last_error(h), "n_streams"));
    htm_classifier_config c = small;
    c.struct_bytes -= 4;
    CHECK(htm_classifiers_create(h, &c, table.data(), N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    c = config(0, {1}, 655, C * K, K, pairs);
    CHECK(htm_classifiers_create(h, &c, table.data(), N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_classifiers_create(h, &small, table.data(), N, nullptr, &bank) == HTM_OK && bank);
    CHECK(htm_classifiers_create(h, &small, table.data(), 1, nullptr, &one) == HTM_OK && one);
    CHECK(htm_classifier_create(h, &small, table.data(), &owner) == HTM_OK && owner);
    // shared weights: the config must be the owner's, the owner a one-stream object
    c = config(6, {0, 1, 5}, 655, C * K, K, pairs);
    CHECK(htm_classifiers_create(h, &c, table.data(), N, owner, &sharer) == HTM_ERR_ARGUMENT && !sharer && strstr(htm_last_error(h), "share_weights_of"));
    c = config(5, {0, 1, 6}, 655, C * K, K, pairs);
    CHECK(htm_classifiers_create(h, &c, table.data(), N, owner, &sharer) == HTM_ERR_ARGUMENT && !sharer);
    CHECK(htm_classifiers_create(h, &small, table.data(), N, bank, &sharer) == HTM_ERR_ARGUMENT && !sharer);
    CHECK(htm_classifiers_create(h, &small, table.data(), N, owner, &sharer) == HTM_OK && sharer);
    if (htm_handle *sharded = make_handle(3, 2)) {              // a column-sharded handle: HTM_ERR_STATE everywhere
        htm_classifier *none = nullptr;
        CHECK(htm_classifiers_create(sharded, &small, table.data(), N, nullptr, &none) == HTM_ERR_STATE && !none);
        CHECK(htm_classifiers_reset(bank, sharded, nullptr) == HTM_ERR_STATE);
        htm_destroy(sharded);
    }

    const int32_t rows_probe[5] = {1, 2, 3, 4, 5};
    // ---- update: learning (two launches per step) and frozen (a launch per chunk), device memory being host memory
    const int T = 2 * HTM_CLASSIFIER_CHUNK + 3, H = 3;
    std::vector<int32_t> pair_store((size_t)T * pairs * 2, -1), targets(10, 2), best((size_t)N * T * H * 2), dist((size_t)N * T * H * 5);
    std::vector<uint32_t> reset_bits(1, 0x21u);
    const void *ptab[N] = {pair_store.data(), pair_store.data(), pair_store.data()};
    const int32_t *ttab[N] = {targets.data(), targets.data(), targets.data()};
    const uint32_t *rtab[N] = {reset_bits.data(), reset_bits.data(), reset_bits.data()};
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 9, ttab, 10, 0, rtab, 1, best.data(), dist.data()) == HTM_OK);
    CHECK(htm_classifiers_update(bank, h, ptab, 1, 9, ttab, 10, 9, nullptr, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifiers_update(bank, hs[1], ptab, pairs, T, ttab, 10, 3, rtab, 0, best.data(), dist.data()) == HTM_OK);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 0, ttab, 10, 0, nullptr, 0, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifiers_update(one, h, ptab, pairs, 4, ttab, 10, 0, rtab, 1, best.data(), dist.data()) == HTM_OK);       // (one stream: by value)
    CHECK(htm_classifiers_update(one, h, ptab, pairs, 4, ttab, 10, 0, nullptr, 0, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifier_update(one, h, pair_store.data(), pairs, 4, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifiers_update(sharer, h, ptab, pairs, 5, ttab, 10, 0, rtab, 0, best.data(), dist.data()) == HTM_OK);
    CHECK(htm_classifiers_update(sharer, h, ptab, pairs, 5, ttab, 10, 0, rtab, 1, best.data(), dist.data()) == HTM_ERR_STATE && strstr(htm_last_error(h), "learn"));
    CHECK(htm_classifier_update(bank, h, pair_store.data(), pairs, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(strstr(htm_last_error(h), "htm_classifiers_"));
    {   // a sharer of one stream learns through neither update call: the owner alone writes its table
        htm_classifier *lone = nullptr;
        CHECK(htm_classifiers_create(h, &small, table.data(), 1, owner, &lone) == HTM_OK && lone);
        CHECK(htm_classifiers_update(lone, h, ptab, pairs, 2, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_STATE);
        CHECK(htm_classifier_update(lone, h, pair_store.data(), pairs, 2, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_STATE);
        CHECK(htm_classifiers_update(lone, h, ptab, pairs, 2, ttab, 10, 0, nullptr, 0, best.data(), nullptr) == HTM_OK);
        CHECK(htm_classifier_update(lone, h, pair_store.data(), pairs, 2, targets.data(), 10, 0, nullptr, 0, best.data(), nullptr) == HTM_OK);   // (512 steps' accumulators behind 2)
        CHECK(htm_classifier_write_weights(lone, h, 0, 0, 1, rows_probe) == HTM_ERR_STATE);
        htm_classifier_destroy(lone);
    }
    CHECK(htm_classifiers_update(nullptr, h, ptab, pairs, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, nullptr, ptab, pairs, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, nullptr, pairs, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 1, nullptr, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 1, ttab, 10, 0, nullptr, 1, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    const void *hole[N] = {pair_store.data(), nullptr, pair_store.data()};
    CHECK(htm_classifiers_update(bank, h, hole, pairs, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stream 1"));
    const uint32_t *rhole[N] = {reset_bits.data(), reset_bits.data(), nullptr};
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 1, ttab, 10, 0, rhole, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, 0, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs + 1, 1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, -1, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 1, ttab, 0, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 1, ttab, 10, -1, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);

    // ---- reset, weights, export, import
    const uint8_t flags[N] = {0, 1, 0};
    CHECK(htm_classifiers_reset(bank, h, nullptr) == HTM_OK && htm_classifiers_reset(bank, h, flags) == HTM_OK && htm_classifiers_reset(one, h, flags) == HTM_OK);
    CHECK(htm_classifiers_reset(nullptr, h, nullptr) == HTM_ERR_ARGUMENT && htm_classifiers_reset(bank, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_reset(bank, h) == HTM_ERR_ARGUMENT);
    std::vector<int32_t> rows((size_t)7 * 5), back((size_t)7 * 5, -3);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int32_t)i * 1000 - 9000;
    rows[0] = 1 << 30;
    rows[1] = -(1 << 30);
    CHECK(htm_classifiers_write_weights(bank, h, 2, 2, C * K - 7, 7, rows.data()) == HTM_OK);          // (the last rows of the last table)
    CHECK(htm_classifiers_read_weights(bank, hs[1], 2, 2, C * K - 7, 7, back.data()) == HTM_OK && rows == back);
    CHECK(htm_classifiers_read_weights(bank, h, 1, 2, C * K - 7, 7, back.data()) == HTM_OK);
    for (int32_t x : back) CHECK(x == 0);       // (another stream's rows)
    CHECK(htm_classifiers_read_weights(bank, h, 0, 0, 0, 0, back.data()) == HTM_OK && htm_classifiers_write_weights(bank, h, 0, 0, C * K, 0, rows.data()) == HTM_OK);
    CHECK(htm_classifiers_read_weights(bank, h, 3, 0, 0, 1, back.data()) == HTM_ERR_ARGUMENT && htm_classifiers_read_weights(bank, h, -1, 0, 0, 1, back.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_read_weights(bank, h, 0, 3, 0, 1, back.data()) == HTM_ERR_ARGUMENT && htm_classifiers_read_weights(bank, h, 0, 0, C * K - 6, 7, back.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_read_weights(bank, h, 0, 0, 0, 1, nullptr) == HTM_ERR_ARGUMENT && htm_classifiers_write_weights(bank, h, 0, 0, 2147483647, 7, rows.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_read_weights(bank, h, 0, 0, 1, back.data()) == HTM_ERR_ARGUMENT && htm_classifier_write_weights(bank, h, 0, 0, 1, rows.data()) == HTM_ERR_ARGUMENT);
    rows[3] = (1 << 30) + 1;
    CHECK(htm_classifiers_write_weights(bank, h, 2, 2, C * K - 7, 7, rows.data()) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "2^30"));
    rows[3] = -6000;
    CHECK(htm_classifiers_read_weights(bank, h, 2, 2, C * K - 7, 7, back.data()) == HTM_OK && rows == back);      // (a refused write changed nothing)
    // a sharer reads the owner's table through every stream and refuses to write it
    CHECK(htm_classifier_write_weights(owner, h, 1, 3, 7, rows.data()) == HTM_OK);
    for (int m = 0; m < N; ++m) CHECK(htm_classifiers_read_weights(sharer, h, m, 1, 3, 7, back.data()) == HTM_OK && rows == back);
    CHECK(htm_classifiers_write_weights(sharer, h, 0, 1, 3, 7, rows.data()) == HTM_ERR_STATE);
    const int64_t ring = 6 * (int64_t)pairs * 8, bytes = htm_classifiers_state_bytes(bank);
    CHECK(bytes == 8 + N * 8 + N * ring && htm_classifiers_state_bytes(nullptr) == HTM_ERR_ARGUMENT && htm_classifiers_state_bytes(one) == 16 + ring);
    CHECK(htm_classifiers_state_bytes(one) == htm_classifier_state_bytes(one) && htm_classifiers_state_bytes(sharer) == bytes);
    std::vector<unsigned char> state((size_t)bytes), again((size_t)bytes, 0xff);
    for (size_t i = 8 + N * 8; i < state.size(); ++i) state[i] = (unsigned char)(i * 7);
    int64_t *head = (int64_t *)state.data();
    head[0] = (int64_t)1 << 40;
    head[1] = 77;
    head[2] = 0;
    head[3] = (int64_t)1 << 40;
    CHECK(htm_classifiers_import(bank, h, state.data(), bytes) == HTM_OK);
    CHECK(htm_classifiers_export(bank, hs[1], again.data(), bytes) == HTM_OK && state == again);
    CHECK(htm_classifiers_update(bank, h, ptab, pairs, 4, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifiers_export(bank, h, again.data(), bytes) == HTM_OK && ((int64_t *)again.data())[0] == ((int64_t)1 << 40) + 4);
    CHECK(htm_classifiers_export(bank, h, again.data(), bytes - 8) == HTM_ERR_ARGUMENT && htm_classifiers_export(bank, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_export(nullptr, h, again.data(), bytes) == HTM_ERR_ARGUMENT && htm_classifiers_import(bank, nullptr, state.data(), bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifiers_import(bank, h, state.data(), bytes + 8) == HTM_ERR_ARGUMENT && htm_classifiers_import(bank, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_export(bank, h, again.data(), 16 + ring) == HTM_ERR_ARGUMENT && htm_classifier_import(bank, h, state.data(), 16 + ring) == HTM_ERR_ARGUMENT);
    head[2] = -1;
    CHECK(htm_classifiers_import(bank, h, state.data(), bytes) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stream 1"));
    head[2] = 0;
    head[3] = ((int64_t)1 << 40) + 1;
    CHECK(htm_classifiers_import(bank, h, state.data(), bytes) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stream 2"));
    std::vector<unsigned char> kept((size_t)bytes);
    CHECK(htm_classifiers_export(bank, h, kept.data(), bytes) == HTM_OK && kept == again);        // (a refused import changed nothing)

    // ---- group pattern capture and the classified tick
    {
        const int words = (I + 31) / 32, n_bank = 4, steps = 12;
        std::vector<uint32_t> input((size_t)n_bank * words, 0x00010001u);
        std::vector<htm_step_record> recs((size_t)N * steps);
        std::vector<int32_t> cells((size_t)N * steps * pairs * 2);
        htm_run_record rec[N];
        void *rows_tab[N];
        const uint32_t *banks[N];
        for (int i = 0; i < N; ++i) {
            memset(&rec[i], 0, sizeof(rec[i]));
            rec[i].struct_bytes = sizeof(rec[i]);
            rec[i].records = recs.data() + (size_t)i * steps;
            rows_tab[i] = cells.data() + (size_t)i * steps * pairs * 2;
            banks[i] = input.data();
        }
        htm_group *g = nullptr;
        CHECK(htm_group_create(hs, N, &g) == HTM_OK && g);
        CHECK(htm_set_group_run_active_cells(nullptr, rows_tab) == HTM_ERR_ARGUMENT);
        void *hole_tab[N] = {rows_tab[0], nullptr, rows_tab[2]};
        CHECK(htm_set_group_run_active_cells(g, hole_tab) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "member 1"));
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 0, nullptr) == HTM_OK);             // (a refused setter set nothing)
        CHECK(htm_set_group_run_active_cells(g, rows_tab) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, steps, 1, 1, rec) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, steps, 0, 0, rec) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 1, nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "htm_set_group_run_active_cells"));
        std::vector<uint32_t> packed((size_t)N * words, 1u);
        CHECK(htm_group_step(g, packed.data(), 1, nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_group_step(g, packed.data(), 1, rec) == HTM_OK);
        const void *cell_tab[N] = {rows_tab[0], rows_tab[1], rows_tab[2]};
        CHECK(htm_classifiers_update(bank, h, cell_tab, pairs, steps, ttab, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
        CHECK(htm_set_group_run_active_cells(g, nullptr) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 0, nullptr) == HTM_OK);
        // a member with rows of its own still makes the group call HTM_ERR_STATE
        CHECK(htm_set_run_active_cells(hs[1], cells.data()) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 0, rec) == HTM_ERR_STATE);
        CHECK(htm_set_run_active_cells(hs[1], nullptr) == HTM_OK);

        // the classified tick: packed rows and values, learning and frozen, scored, with a distribution and without
        std::vector<htm_live_row> live(N);
        std::vector<uint8_t> resets = {1, 0, 1};
        std::vector<int32_t> tg = {0, 4, -1}, tbest((size_t)N * H * 2, -5), tdist((size_t)N * H * 5, -5);
        htm_scalar_field field;
        memset(&field, 0, sizeof(field));
        field.minimum = 0.0;
        field.scale = 0.5;
        field.offset = 0;
        field.bits = 64;
        field.width = 9;
        field.buckets = 56;
        std::vector<double> vals = {1.0, 50.0, 99.0}, lik(N, -1.0);
        std::vector<int32_t> decoded((size_t)N * 2);
        for (int learn = 1; learn >= 0; --learn) {
            for (int graph = 0; graph <= 1; ++graph) {
                CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), resets.data(), 1, graph, live.data(), nullptr, nullptr, nullptr, nullptr, bank, tg.data(),
                                           learn, tbest.data(), nullptr) == HTM_OK);
                CHECK(htm_classifiers_tick(g, vals.data(), &field, 1, nullptr, nullptr, 1, graph, live.data(), decoded.data(), nullptr, nullptr, nullptr, bank, tg.data(),
                                           learn, tbest.data(), tdist.data()) == HTM_OK);     // (the result block grows for the distribution)
            }
        }
        CHECK(tbest[0] == 0 && tdist[0] == 0);          // (zeroes of the stub's device memory: the outputs were copied from the block)
        htm_likelihood_config lcfg;
        memset(&lcfg, 0, sizeof(lcfg));
        lcfg.struct_bytes = sizeof(lcfg);
        lcfg.learning_period = 4;
        lcfg.estimation_samples = 4;
        lcfg.history = 16;
        lcfg.averaging_window = 3;
        lcfg.reestimation_period = 2;
        std::vector<double> tail(513, 0.5);
        htm_likelihood *lk = nullptr;
        CHECK(htm_likelihood_create(h, &lcfg, tail.data(), N, &lk) == HTM_OK && lk);
        std::vector<int32_t> votes((size_t)N * I);
        CHECK(htm_classifiers_tick(g, vals.data(), &field, 1, nullptr, resets.data(), 1, 1, live.data(), decoded.data(), votes.data(), lk, lik.data(), bank, tg.data(), 1,
                                   tbest.data(), tdist.data()) == HTM_OK);
        CHECK(htm_classifiers_tick(g, vals.data(), &field, 1, nullptr, nullptr, 1, 1, live.data(), decoded.data(), nullptr, lk, lik.data(), nullptr, nullptr, 0, nullptr,
                                   nullptr) == HTM_OK);                                        // (htm_likelihood_tick)
        CHECK(htm_likelihood_tick(g, vals.data(), &field, 1, nullptr, nullptr, 1, 1, live.data(), decoded.data(), nullptr, lk, lik.data()) == HTM_OK);
        CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr) == HTM_OK);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 0, 0, live.data(), nullptr, nullptr, nullptr, nullptr, sharer, tg.data(), 0, tbest.data(),
                                   nullptr) == HTM_OK);
        // the refusals: nothing enqueued, the group usable
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 0, 0, live.data(), nullptr, nullptr, nullptr, nullptr, sharer, tg.data(), 1, tbest.data(),
                                   nullptr) == HTM_ERR_STATE && strstr(htm_group_last_error(g), "learn"));
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, bank, tg.data(), 1, nullptr,
                                   nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, tbest.data(),
                                   nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                   tdist.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, bank, nullptr, 1, tbest.data(),
                                   nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, one, tg.data(), 1, tbest.data(),
                                   nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "streams"));
        htm_classifier *thin = nullptr, *other_shape = nullptr;
        c = config(5, {1}, 655, C * K, K, pairs - 1);
        CHECK(htm_classifiers_create(h, &c, table.data(), N, nullptr, &thin) == HTM_OK);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, thin, tg.data(), 1, tbest.data(),
                                   nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "pairs"));
        c = config(5, {1}, 655, C * 32, 32, pairs);
        CHECK(htm_classifiers_create(h, &c, table.data(), N, nullptr, &other_shape) == HTM_OK);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, other_shape, tg.data(), 1,
                                   tbest.data(), nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(nullptr, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, bank, tg.data(), 1,
                                   tbest.data(), nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_classifiers_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, live.data(), nullptr, nullptr, nullptr, nullptr, bank, tg.data(), 1, tbest.data(),
                                   nullptr) == HTM_OK);
        htm_classifier_destroy(thin);
        htm_classifier_destroy(other_shape);
        htm_likelihood_destroy(lk);
        htm_group_destroy(g);
        if (htm_handle *tm_only = make_handle(5, 1, 0)) {       // a member without the device's own Spatial Pooler
            htm_group *lone = nullptr;
            if (htm_group_create(&tm_only, 1, &lone) == HTM_OK && lone) {
                CHECK(htm_set_group_run_active_cells(lone, rows_tab) == HTM_ERR_STATE);
                htm_group_destroy(lone);
            }
            htm_destroy(tm_only);
        }
    }

    // ---- destroy: the owner of shared weights before its sharer, a bank after the handles are gone
    htm_classifier *sharer2 = nullptr;
    CHECK(htm_classifiers_create(h, &small, table.data(), 2, owner, &sharer2) == HTM_OK && sharer2);
    htm_classifier_destroy(sharer2);                    // (a sharer first: the owner's table stays)
    CHECK(htm_classifier_read_weights(owner, h, 1, 3, 7, back.data()) == HTM_OK && rows == back);
    htm_classifier_destroy(owner);                      // (the owner first: the table lives on with the sharer)
    for (int m = 0; m < N; ++m) CHECK(htm_classifiers_read_weights(sharer, h, m, 1, 3, 7, back.data()) == HTM_OK && rows == back);
    CHECK(htm_classifiers_update(sharer, h, ptab, pairs, 5, ttab, 10, 0, rtab, 0, best.data(), dist.data()) == HTM_OK);
    htm_classifier_destroy(sharer);
    htm_classifier_destroy(one);
    for (htm_handle *x : hs) htm_destroy(x);
    htm_classifier_destroy(bank);

    if (argc > 1) arithmetic(argv[1]);
    puts("ok");
    return 0;
}
