// The host code of the KNN classifier under AddressSanitizer + UBSan, as a stand-alone program (tests/test_knn_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_knn_create, _labels, _update,
// _reset, _info, _export, _import and _destroy through the C ABI, with every refusal (each must leave the objects usable).  With a
// file name as its argument it then evaluates the arithmetic of bithtm_amd/csrc/htm_knn.h -- the functions the kernels and the
// host code call, compiled here for the host -- over the cases of that file and prints every result; the test compares them with
// bithtm_amd/knn.py and the constants of bithtm_amd/_lib.py, exactly.
//   o <a> <b>                           -> the bits two words share
//   l <index> <word> <K> <WPC> <cols>   -> the live bits
//   t <cols> <WPC>                      -> words of a table, 1 where the tables lie in LDS, queries a block stages, 1 where the global
//                                          form stages presence bitmaps, the distance launch's dynamic LDS in bytes
//   r <block> <count>                   -> blocks of the distance launch, the block's first slot, the slot behind its last
//   g <nq> <queries>                    -> block rows of the distance launch
//   s <max_pairs> <K>                   -> the largest overlap, the bins' shift
//   n <overlap> <shift>                 -> the overlap's bin, its place inside the bin
//   w <count>                           -> slots of one wave's share of the select's walk
// Exit status 0 and "ok" as the last line on success.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"
#include "../../bithtm_amd/csrc/htm_knn.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48, WPC = 2;

static htm_handle *make_handle(uint32_t seed, int shard_world = 1, int shared_stream = 1) {
    htm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_bytes = sizeof(cfg);
    cfg.input_dim = I;
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
    cfg.segment_capacity = 4096;
    cfg.segment_slots = 64;
    cfg.seed = seed;
    cfg.use_caller_stream = shared_stream;      // (1 with a NULL stream: the default stream; 0: a stream of its own)
    cfg.shard_world = shard_world;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (shard_world > 1 && rc != HTM_OK) return nullptr;
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static htm_knn_config config(int labels, int k, int min_overlap, int capacity, int units, int cell_dim, int max_pairs) {
    htm_knn_config c;
    memset(&c, 0, sizeof(c));
    c.struct_bytes = sizeof(c);
    c.labels = labels;
    c.k = k;
    c.min_overlap = min_overlap;
    c.capacity = capacity;
    c.units = units;
    c.cell_dim = cell_dim;
    c.max_pairs = max_pairs;
    return c;
}

static htm_knn_info_t info_of(const htm_knn *knn) {
    htm_knn_info_t out;
    memset(&out, 0, sizeof(out));
    out.struct_bytes = sizeof(out);
    CHECK(htm_knn_info(knn, &out) == HTM_OK);
    return out;
}

static void arithmetic(const char *path) {
    FILE *f = fopen(path, "r");
    CHECK(f);
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'o') {
            uint32_t a, b;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNu32, &a, &b) == 2);
            printf("%d\n", knn_pair_overlap(a, b));
        } else if (kind[0] == 'l') {
            int32_t index;
            uint32_t word;
            int k, wpc, cols;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNu32 " %d %d %d", &index, &word, &k, &wpc, &cols) == 5);
            printf("%" PRIu32 "\n", cls_live_bits(index, word, k, wpc, cols));
        } else if (kind[0] == 't') {
            int cols, wpc;
            CHECK(fscanf(f, "%d %d", &cols, &wpc) == 2);
            const int64_t words = knn_table_words(cols, wpc);
            printf("%" PRId64 " %d %d %d %" PRId64 "\n", words, knn_in_lds(words), knn_queries(words), knn_has_bitmap(words), knn_distance_lds(words));
        } else if (kind[0] == 'r') {
            int block, count;
            CHECK(fscanf(f, "%d %d", &block, &count) == 2);
            printf("%d %d %d\n", knn_slot_blocks(count), knn_block_first(block), knn_block_last(block, count));
        } else if (kind[0] == 'g') {
            int nq, queries;
            CHECK(fscanf(f, "%d %d", &nq, &queries) == 2);
            printf("%d\n", knn_query_groups(nq, queries));
        } else if (kind[0] == 's') {
            int max_pairs, k;
            CHECK(fscanf(f, "%d %d", &max_pairs, &k) == 2);
            printf("%d %d\n", knn_max_overlap(max_pairs, k), knn_shift(knn_max_overlap(max_pairs, k)));
        } else if (kind[0] == 'n') {
            int overlap, shift;
            CHECK(fscanf(f, "%d %d", &overlap, &shift) == 2);
            printf("%d %d\n", knn_bin(overlap, shift), overlap & ((1 << shift) - 1));
        } else if (kind[0] == 'w') {
            int count;
            CHECK(fscanf(f, "%d", &count) == 1);
            printf("%d\n", knn_wave_span(count));
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    htm_handle *h = make_handle(7), *h2 = make_handle(8);
    const int pairs = ACTIVE * WPC;
    const htm_knn_config small = config(5, 3, 2, 40, C * K, K, pairs);

    // ---- create: refusals, then objects
    htm_knn *knn = nullptr, *big = nullptr, *bad = (htm_knn *)1;
    CHECK(htm_knn_create(nullptr, &small, &knn) == HTM_ERR_ARGUMENT && !knn);
    CHECK(htm_knn_create(h, nullptr, &knn) == HTM_ERR_ARGUMENT && !knn);
    CHECK(htm_knn_create(h, &small, nullptr) == HTM_ERR_ARGUMENT);
    htm_knn_config c = small;
    c.struct_bytes -= 4;
    CHECK(htm_knn_create(h, &c, &bad) == HTM_ERR_ARGUMENT && !bad);
    const htm_knn_config out_of_range[] = {
        config(0, 3, 2, 40, C * K, K, pairs), config(1025, 3, 2, 40, C * K, K, pairs), config(5, 0, 2, 40, C * K, K, pairs), config(5, 65, 2, 40, C * K, K, pairs),
        config(5, 3, 0, 40, C * K, K, pairs), config(5, 3, 65536, 40, C * K, K, pairs), config(5, 3, 2, 0, C * K, K, pairs),
        config(5, 3, 2, (1 << 20) + 1, C * K, K, pairs), config(5, 3, 2, 40, C * K + 1, K, pairs), config(5, 3, 2, 40, 0, K, pairs),
        config(5, 3, 2, 40, C * K, 0, pairs), config(5, 3, 2, 40, 65 * 8, 65, pairs), config(5, 3, 2, 40, C * K, K, 0), config(5, 3, 2, 40, C * K, K, 2048)};
    for (const htm_knn_config &p : out_of_range) {
        CHECK(htm_knn_create(h, &p, &knn) == HTM_ERR_ARGUMENT && !knn);
        CHECK(strlen(htm_last_error(h)) > 0);
    }
    CHECK(htm_knn_create(h, &small, &knn) == HTM_OK && knn);
    c = config(1024, 64, 65535, 300, 14000 * 4, 4, 2047);      // the most labels, neighbours and pairs; tables in the global scratch table
    CHECK(htm_knn_create(h, &c, &big) == HTM_OK && big);
    htm_knn_info_t info = info_of(knn), wide = info_of(big);
    CHECK(info.labels == 5 && info.k == 3 && info.min_overlap == 2 && info.capacity == 40 && info.units == C * K && info.cell_dim == K && info.max_pairs == pairs);
    CHECK(info.count == 0 && info.total == 0 && info.state_bytes == 16 && info.table_in_lds == 1 && info.queries_per_block == HTM_KNN_QUERIES);
    CHECK(info.bin_shift == knn_shift(pairs * 32) && info.bin_shift == 1 && info.device_bytes >= (int64_t)40 * (pairs * 8 + 12 + HTM_KNN_CHUNK * 2));
    CHECK(wide.table_in_lds == 0 && wide.bin_shift == 2 && wide.queries_per_block == HTM_KNN_QUERIES);
    CHECK(wide.device_bytes >= (int64_t)HTM_KNN_CHUNK * 14000 * 4);
    htm_knn_info_t wrong = info;
    wrong.struct_bytes = 8;
    CHECK(htm_knn_info(knn, &wrong) == HTM_ERR_ARGUMENT && htm_knn_info(nullptr, &info) == HTM_ERR_ARGUMENT && htm_knn_info(knn, nullptr) == HTM_ERR_ARGUMENT);
    if (htm_handle *sharded = make_handle(3, 2)) {              // a column-sharded handle: HTM_ERR_STATE everywhere
        htm_knn *none = nullptr;
        CHECK(htm_knn_create(sharded, &small, &none) == HTM_ERR_STATE && !none);
        CHECK(htm_knn_reset(knn, sharded) == HTM_ERR_STATE);
        htm_destroy(sharded);
    }

    // ---- labels and update, device memory being host memory: a call that stores (two launches, then two per chunk), a frozen one
    const int T = 2 * HTM_KNN_CHUNK + 3;
    std::vector<int32_t> pair_store((size_t)T * pairs * 2, -1), best((size_t)T * 5), votes((size_t)T * 1024);
    std::vector<int32_t> host_labels = {0, -1, 4, 5, 2, -7, 1, 1, 0, 3};    // (5 and -7 are no labels: seven of ten are)
    const int32_t *dev_labels = nullptr, *none = (const int32_t *)1;
    CHECK(htm_knn_labels(nullptr, h, host_labels.data(), 10, &dev_labels) == HTM_ERR_ARGUMENT && htm_knn_labels(knn, nullptr, host_labels.data(), 10, &dev_labels) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_labels(knn, h, nullptr, 10, &none) == HTM_ERR_ARGUMENT && !none);
    CHECK(htm_knn_labels(knn, h, host_labels.data(), 0, &dev_labels) == HTM_ERR_ARGUMENT && htm_knn_labels(knn, h, host_labels.data(), 10, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_labels(knn, h, host_labels.data(), 10, &dev_labels) == HTM_OK && dev_labels);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 10, dev_labels, 10, 0, 1, best.data(), votes.data()) == HTM_OK);
    CHECK(info_of(knn).count == 7 && info_of(knn).total == 10 && info_of(knn).state_bytes == 16 + 7 * (pairs * 8 + 12));
    CHECK(htm_knn_update(knn, h2, pair_store.data(), 1, T, dev_labels, 10, 3, 0, best.data(), nullptr) == HTM_OK);      // (frozen: stores nothing)
    CHECK(info_of(knn).count == 7 && info_of(knn).total == 10 + T);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 0, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK);
    // a frozen call may read any labels; a learning one only those of htm_knn_labels
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 4, host_labels.data(), 10, 0, 0, best.data(), nullptr) == HTM_OK);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 4, host_labels.data(), 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "htm_knn_labels"));
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 4, dev_labels, 9, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(nullptr, h, pair_store.data(), pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, nullptr, pair_store.data(), pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, nullptr, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 1, nullptr, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 1, dev_labels, 10, 0, 1, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), 0, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs + 1, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "max_pairs"));
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, -1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 1, dev_labels, 0, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 1, dev_labels, 10, -1, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    const int64_t total_now = info_of(knn).total;
    // capacity 40, 7 in use: 48 steps from row 0 would store 4 * 7 + 5 = 33 (fits exactly); 49 steps one more (refused, nothing changes)
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 49, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_CAPACITY && strstr(htm_last_error(h), "capacity"));
    CHECK(info_of(knn).count == 7 && info_of(knn).total == total_now);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 48, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK && info_of(knn).count == 40);
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 2, dev_labels, 10, 1, 1, best.data(), nullptr) == HTM_ERR_CAPACITY);     // (rows 1, 2: one label)
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 1, dev_labels, 10, 1, 1, best.data(), nullptr) == HTM_OK);                // (row 1: none)
    // the object with the global table: the scatter, distance, select and clear launches of three chunks, 1024 labels of votes
    CHECK(htm_knn_labels(big, h, host_labels.data(), 10, &dev_labels) == HTM_OK);
    std::vector<int32_t> wide_pairs((size_t)T * 2047 * 2, -1);
    CHECK(htm_knn_update(big, h, wide_pairs.data(), 2047, T, dev_labels, 10, 0, 1, best.data(), votes.data()) == HTM_OK && info_of(big).count == 105);        // (eight of ten rows are labels here)
    CHECK(htm_knn_labels(knn, h, host_labels.data(), 3, &dev_labels) == HTM_OK);        // (fewer labels: the array is kept)

    // ---- reset, export, import
    std::vector<unsigned char> state((size_t)info_of(knn).state_bytes), again(state.size(), 0xff);
    CHECK(state.size() == (size_t)16 + 40 * (pairs * 8 + 12));
    CHECK(htm_knn_export(knn, h, state.data(), (int64_t)state.size()) == HTM_OK && ((int64_t *)state.data())[1] == 40);
    CHECK(htm_knn_export(knn, h, state.data(), (int64_t)state.size() - 4) == HTM_ERR_ARGUMENT && htm_knn_export(knn, h, nullptr, 16) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_export(nullptr, h, state.data(), 16) == HTM_ERR_ARGUMENT && htm_knn_export(knn, nullptr, state.data(), 16) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_reset(knn, h) == HTM_OK && info_of(knn).count == 0 && info_of(knn).state_bytes == 16 && info_of(knn).total == ((int64_t *)state.data())[0]);
    CHECK(htm_knn_reset(nullptr, h) == HTM_ERR_ARGUMENT && htm_knn_reset(knn, nullptr) == HTM_ERR_ARGUMENT);
    // a state of three slots, built here: total 9; stamps 2, 5, 8; labels 0, 4, 1
    const size_t three = 16 + 3 * ((size_t)pairs * 8 + 12);
    std::vector<unsigned char> made(three, 0);
    int64_t *head = (int64_t *)made.data();
    head[0] = 9;
    head[1] = 3;
    int64_t stamps[3] = {2, 5, 8};
    int32_t labels3[3] = {0, 4, 1};
    for (size_t i = 16; i < 16 + (size_t)3 * pairs * 8; ++i) made[i] = (unsigned char)(i * 7);
    memcpy(made.data() + 16 + 3 * pairs * 8, stamps, 24);
    memcpy(made.data() + 16 + 3 * pairs * 8 + 24, labels3, 12);
    CHECK(htm_knn_import(knn, h, made.data(), (int64_t)three) == HTM_OK && info_of(knn).count == 3 && info_of(knn).total == 9);
    again.assign(three, 0xff);
    CHECK(htm_knn_export(knn, h2, again.data(), (int64_t)three) == HTM_OK && made == again);
    CHECK(htm_knn_import(knn, h, made.data(), (int64_t)three + 8) == HTM_ERR_ARGUMENT && htm_knn_import(knn, h, nullptr, (int64_t)three) == HTM_ERR_ARGUMENT);
    CHECK(htm_knn_import(knn, nullptr, made.data(), (int64_t)three) == HTM_ERR_ARGUMENT && htm_knn_import(knn, h, made.data(), 8) == HTM_ERR_ARGUMENT);
    std::vector<unsigned char> broken = made;
    ((int64_t *)broken.data())[1] = 41;                          // (count above capacity)
    CHECK(htm_knn_import(knn, h, broken.data(), (int64_t)three) == HTM_ERR_ARGUMENT);
    broken = made;
    ((int64_t *)broken.data())[0] = 8;                           // (a stamp at total)
    CHECK(htm_knn_import(knn, h, broken.data(), (int64_t)three) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stamps"));
    broken = made;
    stamps[1] = 2;                                               // (stamps that do not ascend)
    memcpy(broken.data() + 16 + 3 * pairs * 8, stamps, 24);
    CHECK(htm_knn_import(knn, h, broken.data(), (int64_t)three) == HTM_ERR_ARGUMENT);
    broken = made;
    labels3[2] = 5;                                              // (a label at `labels`)
    memcpy(broken.data() + 16 + 3 * pairs * 8 + 24, labels3, 12);
    CHECK(htm_knn_import(knn, h, broken.data(), (int64_t)three) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "label"));
    CHECK(htm_knn_export(knn, h, again.data(), (int64_t)three) == HTM_OK && made == again);      // (a refused import changed nothing)
    CHECK(htm_knn_update(knn, h, pair_store.data(), pairs, 4, dev_labels, 3, 0, 1, best.data(), votes.data()) == HTM_OK && info_of(knn).count == 6);

    // ---- with a recorded run's captured patterns, next to a classifier's update over the same rows
    {
        const int words = (I + 31) / 32, n_bank = 4, steps = 12;
        std::vector<uint32_t> bank((size_t)n_bank * words, 0x00010001u);
        std::vector<htm_step_record> recs(steps);
        std::vector<int32_t> cells((size_t)steps * pairs * 2);
        htm_run_record rec;
        memset(&rec, 0, sizeof(rec));
        rec.struct_bytes = sizeof(rec);
        rec.records = recs.data();
        CHECK(htm_set_run_active_cells(h, cells.data()) == HTM_OK);
        CHECK(htm_run_recorded(h, bank.data(), n_bank, steps, 1, 1, &rec) == HTM_OK);
        CHECK(htm_set_run_active_cells(h, nullptr) == HTM_OK);
        CHECK(htm_knn_update(knn, h, cells.data(), pairs, steps, dev_labels, 3, 0, 0, best.data(), nullptr) == HTM_OK);
    }

    // ---- an object outlives the handle it was created through
    {
        htm_handle *first = make_handle(31, 1, 0);      // (on a stream of its own, which htm_destroy destroys)
        htm_knn *roaming = nullptr;
        CHECK(htm_knn_create(first, &small, &roaming) == HTM_OK && roaming);
        CHECK(htm_knn_labels(roaming, first, host_labels.data(), 10, &dev_labels) == HTM_OK);
        CHECK(htm_knn_update(roaming, first, pair_store.data(), pairs, 9, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK);
        htm_destroy(first);
        CHECK(htm_knn_update(roaming, h, pair_store.data(), pairs, 5, dev_labels, 10, 0, 0, best.data(), votes.data()) == HTM_OK);
        CHECK(htm_knn_reset(roaming, h2) == HTM_OK);
        htm_knn_destroy(roaming);
    }

    // ---- destroy: an object before its handle, one after the handles are gone
    htm_knn_destroy(big);
    htm_knn_destroy(nullptr);
    htm_destroy(h);
    htm_destroy(h2);
    htm_knn_destroy(knn);

    if (argc > 1) arithmetic(argv[1]);
    puts("ok");
    return 0;
}
