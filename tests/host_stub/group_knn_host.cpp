// The host code of the KNN classifier banks under AddressSanitizer + UBSan, as a stand-alone program (tests/test_group_knn_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_knns_create, _labels, _update,
// _reset, _info, _export, _import and _tick through the C ABI, with every refusal (each must leave the objects usable), and the
// one-stream calls on a bank.  With a file name as its argument it then evaluates the host arithmetic of
// bithtm_amd/csrc/htm_knn_bank.h over the cases of that file and prints every result; the test compares them with its twins, exactly.
//   c <n> <capacity> <words>            -> the chunk of a bank of n own stores, of n streams over a shared store, the scratch bytes at the first
//   o <m> <per>                         -> member m's offset
//   g <n> <nq> <queries> <count>        -> x and y of the distance launch
// Exit status 0 and "ok" as the last line on success.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"
#include "../../bithtm_amd/csrc/htm_knn_bank.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48, WPC = 2;

static htm_handle *make_handle(uint32_t seed, int shard_world = 1) {
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
    cfg.use_caller_stream = 1;
    cfg.shard_world = shard_world;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (shard_world > 1 && rc != HTM_OK) return nullptr;
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

static htm_knns_info_t info_of(const htm_knn *knn, int32_t *counts = nullptr) {
    htm_knns_info_t out;
    memset(&out, 0, sizeof(out));
    out.struct_bytes = sizeof(out);
    CHECK(htm_knns_info(knn, &out, counts) == HTM_OK);
    return out;
}

static void arithmetic(const char *path) {
    FILE *f = fopen(path, "r");
    CHECK(f);
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'c') {
            int64_t n, capacity, words;
            CHECK(fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64, &n, &capacity, &words) == 3);
            const int chunk = gknn_chunk(n, capacity, words);
            printf("%d %d %" PRId64 "\n", chunk, gknn_shared_chunk(n, capacity, words), gknn_scratch_bytes(n, chunk, capacity, words));
        } else if (kind[0] == 'o') {
            int64_t m, per;
            CHECK(fscanf(f, "%" SCNd64 " %" SCNd64, &m, &per) == 2);
            printf("%" PRId64 "\n", gknn_offset(m, per));
        } else if (kind[0] == 'g') {
            int n, nq, queries, count;
            CHECK(fscanf(f, "%d %d %d %d", &n, &nq, &queries, &count) == 4);
            printf("%d %d\n", knn_slot_blocks(count), gknn_distance_rows(n, nq, queries));
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    htm_handle *h = make_handle(7), *h2 = make_handle(8);
    const int pairs = ACTIVE * WPC, N = 3;
    const htm_knn_config small = config(5, 3, 2, 40, C * K, K, pairs);

    // ---- create: refusals, then banks
    htm_knn *bank = nullptr, *wide = nullptr, *bad = (htm_knn *)1, *solo = nullptr, *views = nullptr;
    CHECK(htm_knns_create(nullptr, &small, N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_knns_create(h, nullptr, N, nullptr, &bank) == HTM_ERR_ARGUMENT && htm_knns_create(h, &small, N, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    htm_knn_config c = small;
    c.struct_bytes -= 4;
    CHECK(htm_knns_create(h, &c, N, nullptr, &bad) == HTM_ERR_ARGUMENT && !bad);
    c = config(5, 3, 2, 0, C * K, K, pairs);
    CHECK(htm_knns_create(h, &c, N, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    CHECK(htm_knns_create(h, &small, 0, nullptr, &bank) == HTM_ERR_ARGUMENT && htm_knns_create(h, &small, 65536, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank);
    c = config(5, 3, 2, 1 << 20, 70000 * 4, 4, 8);                // one step's scratch of 65 535 such streams is far past the budget
    CHECK(gknn_chunk(65535, 1 << 20, 70000) == 0);
    CHECK(htm_knns_create(h, &c, 65535, nullptr, &bank) == HTM_ERR_ARGUMENT && !bank && strstr(htm_last_error(h), "scratch"));
    CHECK(htm_knns_create(h, &small, N, nullptr, &bank) == HTM_OK && bank);
    c = config(1024, 64, 65535, 300, 14000 * 4, 4, 2047);         // tables in the global scratch table
    CHECK(htm_knns_create(h, &c, 2, nullptr, &wide) == HTM_OK && wide);
    CHECK(htm_knn_create(h, &small, &solo) == HTM_OK && solo);
    // a shared store: of another config, of a bank -- refused; of a one-stream object of the same config
    CHECK(htm_knns_create(h, &c, 4, solo, &views) == HTM_ERR_ARGUMENT && !views && strstr(htm_last_error(h), "config"));
    CHECK(htm_knns_create(h, &small, 4, bank, &views) == HTM_ERR_ARGUMENT && !views && strstr(htm_last_error(h), "bank"));
    CHECK(htm_knns_create(h, &small, 9, solo, &views) == HTM_OK && views);
    int32_t counts[16];
    htm_knns_info_t info = info_of(bank, counts), shared = info_of(views), global = info_of(wide);
    CHECK(info.n_streams == N && info.shared == 0 && info.chunk == HTM_KNN_CHUNK && info.max_count == 0 && info.total == 0 && info.state_bytes == 8 * (1 + N));
    CHECK(counts[0] == 0 && counts[2] == 0 && info.capacity == 40 && info.max_pairs == pairs && info.table_in_lds == 1);
    CHECK(info.scratch_bytes == gknn_scratch_bytes(N, HTM_KNN_CHUNK, 40, (int64_t)C * WPC) && info.device_bytes >= info.scratch_bytes + (int64_t)N * 40 * (pairs * 8 + 12));
    CHECK(shared.n_streams == 9 && shared.shared == 1 && shared.chunk == HTM_KNN_CHUNK && shared.state_bytes == 8 * 10);
    CHECK(shared.device_bytes < (int64_t)40 * pairs * 8 + shared.scratch_bytes);       // (no store of its own)
    CHECK(global.table_in_lds == 0 && global.chunk == HTM_KNN_CHUNK && global.scratch_bytes == 2ll * 64 * (300 * 2 + 14000 * 4));
    htm_knns_info_t wrong = info;
    wrong.struct_bytes = 8;
    CHECK(htm_knns_info(bank, &wrong, nullptr) == HTM_ERR_ARGUMENT && htm_knns_info(nullptr, &info, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_info(bank, nullptr, nullptr) == HTM_ERR_ARGUMENT && htm_knns_info(solo, &info, nullptr) == HTM_ERR_ARGUMENT);
    if (htm_handle *sharded = make_handle(3, 2)) {
        htm_knn *none = nullptr;
        CHECK(htm_knns_create(sharded, &small, N, nullptr, &none) == HTM_ERR_STATE && !none);
        CHECK(htm_knns_reset(bank, sharded, nullptr) == HTM_ERR_STATE);
        htm_destroy(sharded);
    }

    // ---- labels and update, device memory being host memory
    const int T = HTM_KNN_CHUNK + 3;
    std::vector<int32_t> pair_store((size_t)9 * T * pairs * 2, -1), best((size_t)9 * T * 5), votes((size_t)9 * T * 1024);
    // rows of ten labels per stream: stream 0 has seven labels, stream 1 none, stream 2 ten
    std::vector<int32_t> host_labels = {0, -1, 4, 5, 2, -7, 1, 1, 0, 3, -1, -1, -1, -1, -1, -1, -1, -1, -1, 9, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2};
    const int32_t *dev_labels = nullptr, *none = (const int32_t *)1;
    const void *rows[9];
    for (int i = 0; i < 9; ++i) rows[i] = pair_store.data() + (size_t)i * T * pairs * 2;
    CHECK(htm_knns_labels(nullptr, h, host_labels.data(), 10, &dev_labels) == HTM_ERR_ARGUMENT && htm_knns_labels(bank, nullptr, host_labels.data(), 10, &dev_labels) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_labels(bank, h, nullptr, 10, &none) == HTM_ERR_ARGUMENT && !none && htm_knns_labels(bank, h, host_labels.data(), 0, &dev_labels) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_labels(solo, h, host_labels.data(), 10, &dev_labels) == HTM_ERR_STATE && htm_knn_labels(bank, h, host_labels.data(), 10, &dev_labels) == HTM_ERR_STATE);
    CHECK(htm_knns_labels(bank, h, host_labels.data(), 10, &dev_labels) == HTM_OK && dev_labels);
    CHECK(htm_knns_update(bank, h, rows, pairs, 10, dev_labels, 10, 0, 1, best.data(), votes.data()) == HTM_OK);
    info = info_of(bank, counts);
    CHECK(counts[0] == 7 && counts[1] == 0 && counts[2] == 10 && info.max_count == 10 && info.total == 10 && info.state_bytes == 8 * (1 + N) + 17 * (pairs * 8 + 12));
    CHECK(htm_knns_update(bank, h2, rows, 1, T, nullptr, 10, 3, 0, best.data(), nullptr) == HTM_OK && info_of(bank).total == 10 + T);        // (frozen: no labels needed)
    CHECK(htm_knns_update(bank, h, rows, pairs, 0, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_knns_update(bank, h, rows, pairs, 4, host_labels.data(), 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "htm_knns_labels"));
    CHECK(htm_knns_update(bank, h, rows, pairs, 4, dev_labels, 9, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, h, rows, pairs, 4, nullptr, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(nullptr, h, rows, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, nullptr, rows, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, h, nullptr, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, h, rows, pairs, 1, dev_labels, 10, 0, 1, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    const void *holed[3] = {rows[0], nullptr, rows[2]};
    CHECK(htm_knns_update(bank, h, holed, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stream 1"));
    CHECK(htm_knns_update(bank, h, rows, 0, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, h, rows, pairs + 1, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "max_pairs"));
    CHECK(htm_knns_update(bank, h, rows, pairs, -1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_update(bank, h, rows, pairs, 1, dev_labels, 10, -1, 1, best.data(), nullptr) == HTM_ERR_ARGUMENT);
    // the one-stream calls on a bank, and the bank's on a one-stream object
    CHECK(htm_knn_update(bank, h, rows[0], pairs, 1, dev_labels, 10, 0, 0, best.data(), nullptr) == HTM_ERR_STATE && htm_knn_reset(bank, h) == HTM_ERR_STATE);
    CHECK(htm_knn_export(bank, h, best.data(), 16) == HTM_ERR_STATE && htm_knn_import(bank, h, best.data(), 16) == HTM_ERR_STATE);
    CHECK(htm_knns_update(solo, h, rows, pairs, 1, nullptr, 10, 0, 0, best.data(), nullptr) == HTM_ERR_STATE && htm_knns_reset(solo, h, nullptr) == HTM_ERR_STATE);
    // capacity 40: stream 2 holds 10 and stores every step; 31 more steps are one too many for it alone -- the whole call is refused
    const int64_t total_now = info_of(bank).total;
    CHECK(htm_knns_update(bank, h, rows, pairs, 31, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_CAPACITY && strstr(htm_last_error(h), "stream 2"));
    info = info_of(bank, counts);
    CHECK(counts[0] == 7 && counts[1] == 0 && counts[2] == 10 && info.total == total_now);
    CHECK(htm_knns_update(bank, h, rows, pairs, 30, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK);
    info_of(bank, counts);
    CHECK(counts[0] == 28 && counts[1] == 0 && counts[2] == 40);
    // the bank with the global table: scatter, distance, select and clear of two chunks; 1024 labels of votes
    CHECK(htm_knns_labels(wide, h, host_labels.data(), 10, &dev_labels) == HTM_OK);
    std::vector<int32_t> wide_pairs((size_t)2 * T * 2047 * 2, -1);
    const void *wide_rows[2] = {wide_pairs.data(), wide_pairs.data() + (size_t)T * 2047 * 2};
    CHECK(htm_knns_update(wide, h, wide_rows, 2047, T, dev_labels, 10, 0, 1, best.data(), votes.data()) == HTM_OK && info_of(wide).max_count > 0);
    // the shared bank: frozen, one flat batch; learning and rows that do not lie one behind the other are refused
    CHECK(htm_knn_labels(solo, h, host_labels.data(), 10, &dev_labels) == HTM_OK);
    CHECK(htm_knn_update(solo, h, rows[0], pairs, 10, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_OK);
    CHECK(htm_knns_update(views, h, rows, pairs, T, nullptr, 1, 0, 0, best.data(), votes.data()) == HTM_OK);
    shared = info_of(views, counts);
    CHECK(shared.total == T && shared.max_count == 7 && counts[0] == 0 && counts[8] == 0);
    CHECK(htm_knns_update(views, h, rows, pairs, 1, dev_labels, 10, 0, 1, best.data(), nullptr) == HTM_ERR_STATE);
    CHECK(htm_knns_update(views, h, rows, pairs, 2, nullptr, 1, 0, 0, best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "one behind the other"));

    // ---- reset, export, import
    std::vector<unsigned char> state((size_t)info_of(bank).state_bytes), again(state.size(), 0xff);
    CHECK(state.size() == (size_t)8 * (1 + N) + 68 * (pairs * 8 + 12));
    CHECK(htm_knns_export(bank, h, state.data(), (int64_t)state.size()) == HTM_OK && ((int64_t *)state.data())[1] == 28 && ((int64_t *)state.data())[3] == 40);
    CHECK(htm_knns_export(bank, h, state.data(), (int64_t)state.size() - 4) == HTM_ERR_ARGUMENT && htm_knns_export(bank, h, nullptr, 64) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_export(nullptr, h, state.data(), 64) == HTM_ERR_ARGUMENT && htm_knns_export(solo, h, state.data(), 64) == HTM_ERR_STATE);
    {   // (kernels do nothing here: the slots' stamps and labels are written as the append launch would have left them)
        const size_t slots[2] = {28, 40};
        unsigned char *stamps = state.data() + 8 * (1 + N) + (size_t)68 * pairs * 8, *labels = stamps + 68 * 8;
        size_t at = 0;
        for (size_t s = 0; s < 2; ++s)
            for (size_t i = 0; i < slots[s]; ++i, ++at) {
                const int64_t stamp = (int64_t)i;
                const int32_t label = (int32_t)(i % 5);
                memcpy(stamps + at * 8, &stamp, 8);
                memcpy(labels + at * 4, &label, 4);
            }
    }
    const uint8_t only_two[3] = {0, 0, 1};
    CHECK(htm_knns_reset(bank, h, only_two) == HTM_OK);
    info = info_of(bank, counts);
    CHECK(counts[0] == 28 && counts[2] == 0 && info.max_count == 28 && info.total == ((int64_t *)state.data())[0]);
    CHECK(htm_knns_reset(bank, h, nullptr) == HTM_OK && info_of(bank).max_count == 0 && info_of(bank).state_bytes == 8 * (1 + N));
    CHECK(htm_knns_reset(nullptr, h, nullptr) == HTM_ERR_ARGUMENT && htm_knns_reset(bank, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_import(bank, h, state.data(), (int64_t)state.size()) == HTM_OK);
    info = info_of(bank, counts);
    CHECK(counts[0] == 28 && counts[1] == 0 && counts[2] == 40 && info.max_count == 40);
    CHECK(htm_knns_export(bank, h2, again.data(), (int64_t)again.size()) == HTM_OK && state == again);
    CHECK(htm_knns_import(bank, h, state.data(), (int64_t)state.size() + 8) == HTM_ERR_ARGUMENT && htm_knns_import(bank, h, nullptr, 64) == HTM_ERR_ARGUMENT);
    CHECK(htm_knns_import(bank, h, state.data(), 8) == HTM_ERR_ARGUMENT);
    std::vector<unsigned char> broken = state;
    ((int64_t *)broken.data())[2] = 41;                         // (stream 1's count above capacity)
    CHECK(htm_knns_import(bank, h, broken.data(), (int64_t)broken.size()) == HTM_ERR_ARGUMENT);
    broken = state;
    ((int64_t *)broken.data())[0] = 5;                          // (stamps at and above total)
    CHECK(htm_knns_import(bank, h, broken.data(), (int64_t)broken.size()) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "stamps"));
    broken = state;
    int32_t five = 5;                                           // (a label at `labels`, in the last slot)
    memcpy(broken.data() + broken.size() - 4, &five, 4);
    CHECK(htm_knns_import(bank, h, broken.data(), (int64_t)broken.size()) == HTM_ERR_ARGUMENT && strstr(htm_last_error(h), "label"));
    CHECK(htm_knns_export(bank, h, again.data(), (int64_t)again.size()) == HTM_OK && state == again);       // (a refused import changed nothing)
    // a sharing bank's state is its total
    int64_t shared_state[10];
    CHECK(htm_knns_export(views, h, shared_state, 80) == HTM_OK && shared_state[0] == T && shared_state[9] == 0);
    shared_state[0] = 3;
    CHECK(htm_knns_import(views, h, shared_state, 80) == HTM_OK && info_of(views).total == 3);
    shared_state[4] = 1;
    CHECK(htm_knns_import(views, h, shared_state, 80) == HTM_ERR_ARGUMENT);

    // ---- ticks of a group of three members
    {
        htm_handle *m[3] = {make_handle(21), make_handle(22), make_handle(23)};
        htm_group *g = nullptr;
        CHECK(htm_group_create(m, 3, &g) == HTM_OK && g);
        const int words = (I + 31) / 32;
        std::vector<uint32_t> packed((size_t)3 * words, 0x00010001u);
        std::vector<htm_live_row> live(3);
        std::vector<int32_t> tick_best(3 * 5), tick_votes(3 * 5);
        int32_t tick_labels[3] = {1, -1, 9};                    // (9 is no label: one stream stores)
        CHECK(htm_knns_reset(bank, h, nullptr) == HTM_OK);
        auto tick = [&](htm_knn *knn, const int32_t *labels, int learn, int32_t *out, int32_t *all) {
            return htm_knns_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr,
                                 nullptr, knn, labels, learn, out, all);
        };
        CHECK(tick(bank, tick_labels, 1, tick_best.data(), tick_votes.data()) == HTM_OK);
        info = info_of(bank, counts);
        CHECK(counts[0] == 1 && counts[1] == 0 && counts[2] == 0 && info.max_count == 1);
        CHECK(tick(bank, nullptr, 0, tick_best.data(), nullptr) == HTM_OK);                                  // (frozen)
        const int64_t ticks = info_of(bank).total;
        CHECK(tick(nullptr, tick_labels, 1, tick_best.data(), nullptr) == HTM_ERR_ARGUMENT && tick(bank, tick_labels, 1, nullptr, nullptr) == HTM_ERR_ARGUMENT);
        CHECK(tick(bank, nullptr, 1, tick_best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "labels"));
        CHECK(tick(solo, tick_labels, 0, tick_best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "one-stream"));
        CHECK(tick(views, nullptr, 0, tick_best.data(), nullptr) == HTM_ERR_ARGUMENT && strstr(htm_group_last_error(g), "9 streams"));
        CHECK(tick(wide, nullptr, 0, tick_best.data(), nullptr) == HTM_ERR_ARGUMENT);                       // (two streams, another shape)
        htm_knn *three_views = nullptr, *tiny = nullptr;
        CHECK(htm_knns_create(h, &small, 3, solo, &three_views) == HTM_OK);
        CHECK(tick(three_views, nullptr, 0, tick_best.data(), tick_votes.data()) == HTM_OK && info_of(three_views).total == 1);
        CHECK(tick(three_views, tick_labels, 1, tick_best.data(), nullptr) == HTM_ERR_STATE);
        c = config(5, 3, 2, 1, C * K, K, pairs);
        CHECK(htm_knns_create(h, &c, 3, nullptr, &tiny) == HTM_OK);
        CHECK(tick(tiny, tick_labels, 1, tick_best.data(), nullptr) == HTM_OK);
        CHECK(tick(tiny, tick_labels, 1, tick_best.data(), nullptr) == HTM_ERR_CAPACITY && strstr(htm_group_last_error(g), "stream 0"));
        CHECK(info_of(tiny).total == 1 && info_of(bank).total == ticks);
        // the classifier's arguments and the bank's go their own ways: a tick without knn through this door is refused
        CHECK(htm_knns_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, live.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr,
                            nullptr, nullptr, 0, nullptr, nullptr) == HTM_ERR_ARGUMENT);
        htm_knn_destroy(tiny);
        htm_knn_destroy(three_views);
        htm_group_destroy(g);
        for (htm_handle *x : m) htm_destroy(x);
    }

    // ---- destroy: the shared store's owner goes before the bank that reads it; the store lives until the bank goes
    htm_knn_destroy(solo);
    const void *tight[9];
    for (int i = 0; i < 9; ++i) tight[i] = pair_store.data() + (size_t)i * pairs * 2;
    CHECK(htm_knns_update(views, h, tight, pairs, 1, nullptr, 1, 0, 0, best.data(), nullptr) == HTM_OK);
    htm_knn_destroy(views);
    htm_knn_destroy(wide);
    htm_destroy(h);
    htm_destroy(h2);
    htm_knn_destroy(bank);
    htm_knn_destroy(nullptr);

    if (argc > 1) arithmetic(argv[1]);
    puts("ok");
    return 0;
}
