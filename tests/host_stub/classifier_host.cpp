// The host code of the SDR classifier under AddressSanitizer + UBSan, as a stand-alone program (tests/test_classifier_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_classifier_create, _update,
// _reset, _read_weights, _write_weights, _state_bytes, _export, _import, _destroy and htm_set_run_active_cells with recorded runs
// through the C ABI, with every refusal (each must leave the objects usable).  With a file name as its argument it then evaluates
// the arithmetic of bithtm_amd/csrc/htm_classifier.h -- the functions the kernels call, compiled here for the host -- over the cases
// of that file and prints every result; the test compares them with bithtm_amd/classifier.py, exactly.
//   T <2049 ints>                       the exp table
//   e <d>                            -> e
//   s <n> <a_0 .. a_(n-1)>           -> best bucket, then p_0 .. p_(n-1)   (the softmax as the kernel forms it: max, e, Z, p)
//   d <alpha_q> <p> <is_target>      -> delta
//   c <w> <delta>                    -> the clamped sum
//   b <index> <word> <K> <WPC> <cols>-> the live bits, and the first unit (or -1 without live bits)
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

static htm_handle *make_handle(uint32_t seed, int shard_world = 1, int shared_stream = 1, int enable_sp = 1) {
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
    cfg.use_caller_stream = shared_stream;      // (1 with a NULL stream: the default stream; 0: a stream of its own)
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
    std::vector<int32_t> table;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'T') {
            table.resize(HTM_CLASSIFIER_EXP);
            for (int32_t &x : table) CHECK(fscanf(f, "%" SCNd32, &x) == 1);
        } else if (kind[0] == 'e') {
            int64_t d;
            CHECK(fscanf(f, "%" SCNd64, &d) == 1 && table.size() == HTM_CLASSIFIER_EXP);
            printf("%" PRId32 "\n", cls_exp(d, table.data()));
        } else if (kind[0] == 's') {
            int n;
            CHECK(fscanf(f, "%d", &n) == 1 && n >= 1 && table.size() == HTM_CLASSIFIER_EXP);
            std::vector<int64_t> a((size_t)n);
            for (int64_t &x : a) CHECK(fscanf(f, "%" SCNd64, &x) == 1);
            int best = 0;
            for (int b = 1; b < n; ++b)
                if (a[b] > a[best]) best = b;
            std::vector<int32_t> e((size_t)n);
            int64_t z = 0;
            for (int b = 0; b < n; ++b) z += e[b] = cls_exp(a[best] - a[b], table.data());
            printf("%d", best);
            for (int b = 0; b < n; ++b) printf(" %" PRId32, cls_prob(e[b], z));
            printf("\n");
        } else if (kind[0] == 'd') {
            int32_t alpha_q, p;
            int is_target;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNd32 " %d", &alpha_q, &p, &is_target) == 3);
            printf("%" PRId32 "\n", cls_delta(alpha_q, p, is_target));
        } else if (kind[0] == 'c') {
            int32_t w, d;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNd32, &w, &d) == 2);
            printf("%" PRId32 "\n", cls_clamp(w, d));
        } else if (kind[0] == 'b') {
            int32_t index;
            uint32_t word;
            int k, wpc, cols;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNu32 " %d %d %d", &index, &word, &k, &wpc, &cols) == 5);
            const uint32_t bits = cls_live_bits(index, word, k, wpc, cols);
            printf("%" PRIu32 " %" PRId64 "\n", bits, bits ? cls_unit0(index, k, wpc) : (int64_t)-1);
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    htm_handle *h = make_handle(7), *h2 = make_handle(8);
    std::vector<int32_t> table(HTM_CLASSIFIER_EXP, 1 << 20);    // exactly 2049: one fewer read is the sanitizer's to report
    const int pairs = ACTIVE * WPC;
    const htm_classifier_config small = config(5, {0, 1, 5}, 655, C * K, K, pairs);

    // ---- create: refusals, then objects
    htm_classifier *clf = nullptr, *wide = nullptr, *bad = (htm_classifier *)1;
    CHECK(htm_classifier_create(nullptr, &small, table.data(), &clf) == HTM_ERR_ARGUMENT && !clf);
    CHECK(htm_classifier_create(h, nullptr, table.data(), &clf) == HTM_ERR_ARGUMENT && !clf);
    CHECK(htm_classifier_create(h, &small, nullptr, &clf) == HTM_ERR_ARGUMENT && !clf);
    CHECK(htm_classifier_create(h, &small, table.data(), nullptr) == HTM_ERR_ARGUMENT);
    htm_classifier_config c = small;
    c.struct_bytes -= 4;
    CHECK(htm_classifier_create(h, &c, table.data(), &bad) == HTM_ERR_ARGUMENT && !bad);
    const htm_classifier_config out_of_range[] = {
        config(0, {1}, 655, C * K, K, pairs), config(1025, {1}, 655, C * K, K, pairs), config(5, {}, 655, C * K, K, pairs),
        config(5, {0, 1, 2, 3, 4, 5, 6, 7, 8}, 655, C * K, K, pairs), config(5, {-1}, 655, C * K, K, pairs), config(5, {65}, 655, C * K, K, pairs),
        config(5, {2, 2}, 655, C * K, K, pairs), config(5, {3, 1}, 655, C * K, K, pairs), config(5, {1}, 0, C * K, K, pairs),
        config(5, {1}, 65537, C * K, K, pairs), config(5, {1}, 655, C * K + 1, K, pairs), config(5, {1}, 655, 0, K, pairs),
        config(5, {1}, 655, C * K, 0, pairs), config(5, {1}, 655, 65 * 8, 65, pairs), config(5, {1}, 655, C * K, K, 0)};
    for (const htm_classifier_config &p : out_of_range) {      // (the one with nine steps holds eight of them and says nine)
        CHECK(htm_classifier_create(h, &p, table.data(), &clf) == HTM_ERR_ARGUMENT && !clf);
        CHECK(strlen(htm_last_error(h)) > 0);
    }
    CHECK(htm_classifier_create(h, &small, table.data(), &clf) == HTM_OK && clf);
    c = config(1024, {0, 1, 2, 3, 5, 8, 13, 64}, 65536, 64 * 5, 5, 1);      // the most buckets and horizons, the longest ring
    CHECK(htm_classifier_create(h, &c, table.data(), &wide) == HTM_OK && wide);
    if (htm_handle *sharded = make_handle(3, 2)) {              // a column-sharded handle: HTM_ERR_STATE everywhere
        htm_classifier *none = nullptr;
        CHECK(htm_classifier_create(sharded, &small, table.data(), &none) == HTM_ERR_STATE && !none);
        CHECK(htm_classifier_reset(clf, sharded) == HTM_ERR_STATE);
        CHECK(htm_set_run_active_cells(sharded, table.data()) == HTM_ERR_STATE);
        htm_destroy(sharded);
    }

    // ---- update: learning (two launches per step) and frozen (a launch per HTM_CLASSIFIER_CHUNK steps), device memory being host memory
    const int T = 2 * HTM_CLASSIFIER_CHUNK + 3;
    std::vector<int32_t> pair_store((size_t)T * pairs * 2, -1), targets(10, 2), best((size_t)T * 3 * 2), dist((size_t)T * 3 * 5);
    std::vector<uint32_t> reset_bits(1, 0x21u);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 9, targets.data(), 10, 0, reset_bits.data(), 1, best.data(), dist.data()) == HTM_OK);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), 1, 9, targets.data(), 10, 9, nullptr, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifier_update(clf, h2, pair_store.data(), pairs, T, targets.data(), 10, 3, reset_bits.data(), 0, best.data(), dist.data()) == HTM_OK);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 0, targets.data(), 10, 0, nullptr, 0, best.data(), nullptr) == HTM_OK);
    std::vector<int32_t> wide_best((size_t)3 * 8 * 2), wide_dist((size_t)3 * 8 * 1024);
    CHECK(htm_classifier_update(wide, h, pair_store.data(), 1, 3, targets.data(), 10, 0, nullptr, 1, wide_best.data(), wide_dist.data()) == HTM_OK);
    CHECK(htm_classifier_update(wide, h, pair_store.data(), 1, 3, targets.data(), 10, 0, nullptr, 0, wide_best.data(), wide_dist.data()) == HTM_OK);
    CHECK(htm_classifier_update(nullptr, h, pair_store.data(), pairs, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, nullptr, pair_store.data(), pairs, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, nullptr, pairs, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 1, nullptr, 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 1, targets.data(), 10, 0, nullptr, 1, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), 0, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs + 1, 1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(strstr(htm_last_error(h), "max_pairs"));
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, -1, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 1, targets.data(), 0, 0, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 1, targets.data(), 10, -1, nullptr, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);

    // ---- reset, weights, export, import
    CHECK(htm_classifier_reset(clf, h) == HTM_OK);
    CHECK(htm_classifier_reset(nullptr, h) == HTM_ERR_ARGUMENT && htm_classifier_reset(clf, nullptr) == HTM_ERR_ARGUMENT);
    std::vector<int32_t> rows((size_t)7 * 5), back((size_t)7 * 5, -3);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int32_t)i * 1000 - 9000;
    rows[0] = 1 << 30;
    rows[1] = -(1 << 30);
    CHECK(htm_classifier_write_weights(clf, h, 2, C * K - 7, 7, rows.data()) == HTM_OK);
    CHECK(htm_classifier_read_weights(clf, h2, 2, C * K - 7, 7, back.data()) == HTM_OK && rows == back);
    CHECK(htm_classifier_read_weights(clf, h, 1, C * K - 7, 7, back.data()) == HTM_OK);
    for (int32_t x : back) CHECK(x == 0);       // (another horizon's rows)
    CHECK(htm_classifier_read_weights(clf, h, 0, 0, 0, back.data()) == HTM_OK && htm_classifier_write_weights(clf, h, 0, C * K, 0, rows.data()) == HTM_OK);
    CHECK(htm_classifier_read_weights(clf, h, 3, 0, 1, back.data()) == HTM_ERR_ARGUMENT && htm_classifier_read_weights(clf, h, -1, 0, 1, back.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_read_weights(clf, h, 0, C * K - 6, 7, back.data()) == HTM_ERR_ARGUMENT && htm_classifier_read_weights(clf, h, 0, -1, 1, back.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_read_weights(clf, h, 0, 0, -1, back.data()) == HTM_ERR_ARGUMENT && htm_classifier_read_weights(clf, h, 0, 0, 1, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_write_weights(clf, h, 0, 2147483647, 7, rows.data()) == HTM_ERR_ARGUMENT && htm_classifier_write_weights(clf, h, 0, 0, 1, nullptr) == HTM_ERR_ARGUMENT);
    rows[3] = (1 << 30) + 1;
    CHECK(htm_classifier_write_weights(clf, h, 2, C * K - 7, 7, rows.data()) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "2^30"));
    rows[3] = -(1 << 30) - 1;
    CHECK(htm_classifier_write_weights(clf, h, 2, C * K - 7, 7, rows.data()) == HTM_ERR_ARGUMENT);
    rows[3] = -6000;
    CHECK(htm_classifier_read_weights(clf, h, 2, C * K - 7, 7, back.data()) == HTM_OK && rows == back);      // (a refused write changed nothing)
    const int64_t bytes = htm_classifier_state_bytes(clf);
    CHECK(bytes == 16 + 6 * pairs * 8 && htm_classifier_state_bytes(nullptr) == HTM_ERR_ARGUMENT && htm_classifier_state_bytes(wide) == 16 + 65 * 8);
    std::vector<unsigned char> state((size_t)bytes), again((size_t)bytes, 0xff);
    for (size_t i = 16; i < state.size(); ++i) state[i] = (unsigned char)(i * 7);
    ((int64_t *)state.data())[0] = (int64_t)1 << 40;
    ((int64_t *)state.data())[1] = 77;
    CHECK(htm_classifier_import(clf, h, state.data(), bytes) == HTM_OK);
    CHECK(htm_classifier_export(clf, h2, again.data(), bytes) == HTM_OK && state == again);
    CHECK(htm_classifier_update(clf, h, pair_store.data(), pairs, 4, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_classifier_export(clf, h, again.data(), bytes) == HTM_OK && ((int64_t *)again.data())[0] == ((int64_t)1 << 40) + 4);
    CHECK(htm_classifier_export(clf, h, again.data(), bytes - 8) == HTM_ERR_ARGUMENT && htm_classifier_export(clf, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_export(nullptr, h, again.data(), bytes) == HTM_ERR_ARGUMENT && htm_classifier_import(clf, nullptr, state.data(), bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_classifier_import(clf, h, state.data(), bytes + 8) == HTM_ERR_ARGUMENT && htm_classifier_import(clf, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    ((int64_t *)state.data())[1] = -1;
    CHECK(htm_classifier_import(clf, h, state.data(), bytes) == HTM_ERR_ARGUMENT);
    ((int64_t *)state.data())[0] = 5;
    ((int64_t *)state.data())[1] = 6;
    CHECK(htm_classifier_import(clf, h, state.data(), bytes) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "count"));
    std::vector<unsigned char> kept((size_t)bytes);
    CHECK(htm_classifier_export(clf, h, kept.data(), bytes) == HTM_OK && kept == again);        // (a refused import changed nothing)

    // ---- pattern capture: rows set, recorded runs with graphs and without, the refusals while they are set, cleared again
    {
        const int words = (I + 31) / 32, n_bank = 4, steps = 12;
        std::vector<uint32_t> bank((size_t)n_bank * words, 0x00010001u);
        std::vector<htm_step_record> recs(steps);
        std::vector<int32_t> cells((size_t)steps * pairs * 2);
        htm_run_record rec;
        memset(&rec, 0, sizeof(rec));
        rec.struct_bytes = sizeof(rec);
        rec.records = recs.data();
        CHECK(htm_set_run_active_cells(nullptr, cells.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_set_run_active_cells(h, cells.data()) == HTM_OK);
        CHECK(htm_run_recorded(h, bank.data(), n_bank, steps, 1, 1, &rec) == HTM_OK);
        CHECK(htm_run_recorded(h, bank.data(), n_bank, steps, 0, 0, &rec) == HTM_OK);
        CHECK(htm_run(h, bank.data(), n_bank, 2, 1, 1) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "htm_set_run_active_cells"));
        CHECK(htm_run_recorded(h, bank.data(), n_bank, 2, 1, 1, nullptr) == HTM_ERR_ARGUMENT);
        std::vector<int32_t> lists((size_t)2 * ACTIVE, 1);
        CHECK(htm_tm_run(h, lists.data(), 2, ACTIVE, 1, 1, 0, nullptr) == HTM_ERR_STATE);
        htm_handle *members[2] = {h, h2};
        htm_group *g = nullptr;
        CHECK(htm_group_create(members, 2, &g) == HTM_OK && g);
        const uint32_t *banks[2] = {bank.data(), bank.data()};
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 0, nullptr) == HTM_ERR_STATE && strstr(htm_group_last_error(g), "htm_set_run_active_cells"));
        CHECK(htm_set_run_active_cells(h, nullptr) == HTM_OK);
        CHECK(htm_group_run(g, banks, n_bank, 2, 1, 0, nullptr) == HTM_OK);
        htm_group_destroy(g);
        CHECK(htm_run(h, bank.data(), n_bank, 2, 1, 1) == HTM_OK);
        CHECK(htm_classifier_update(clf, h, cells.data(), pairs, steps, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
        if (htm_handle *tm_only = make_handle(5, 1, 1, 0)) {    // a handle without the device's own Spatial Pooler
            CHECK(htm_set_run_active_cells(tm_only, cells.data()) == HTM_ERR_STATE);
            htm_destroy(tm_only);
        }
    }

    // ---- an object outlives the handle it was created through
    {
        htm_handle *first = make_handle(31, 1, 0);      // (on a stream of its own, which htm_destroy destroys)
        htm_classifier *roaming = nullptr;
        CHECK(htm_classifier_create(first, &small, table.data(), &roaming) == HTM_OK && roaming);
        CHECK(htm_classifier_update(roaming, first, pair_store.data(), pairs, 9, targets.data(), 10, 0, nullptr, 1, best.data(), nullptr) == HTM_OK);
        htm_destroy(first);
        CHECK(htm_classifier_update(roaming, h, pair_store.data(), pairs, 5, targets.data(), 10, 0, nullptr, 0, best.data(), dist.data()) == HTM_OK);
        CHECK(htm_classifier_reset(roaming, h2) == HTM_OK);
        CHECK(htm_classifier_export(roaming, h2, again.data(), bytes) == HTM_OK);
        htm_classifier_destroy(roaming);
    }

    // ---- destroy: an object before its handle, one after the handles are gone
    htm_classifier_destroy(wide);
    htm_classifier_destroy(nullptr);
    htm_destroy(h);
    htm_destroy(h2);
    htm_classifier_destroy(clf);

    if (argc > 1) arithmetic(argv[1]);
    puts("ok");
    return 0;
}
