// The host code of the anomaly likelihood under AddressSanitizer + UBSan, as a stand-alone program (tests/test_likelihood_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_likelihood_create, _update,
// _reset, _export, _import, _destroy and scored ticks (htm_likelihood_tick) through the C ABI, with every refusal (each must leave
// the objects usable).  With a file name as its argument it then evaluates the arithmetic of bithtm_amd/csrc/htm_likelihood.h --
// the functions the kernel calls, compiled here for the host with -ffp-contract=off as the library is -- over the cases of that
// file and prints every result as the hex of its bits; the test compares them with bithtm_amd/likelihood.py, exactly.
//   T <513 hex doubles>            the tail table
//   q <active> <bursting>       -> the integer q
//   e <n> <s1> <s2>             -> mean std
//   l <a> <hex mean> <hex std>  -> L
// Exit status 0 and "ok" as the last line on success.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"
#include "../../bithtm_amd/csrc/htm_likelihood.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48;

static htm_handle *make_handle(uint32_t seed, int shard_world = 1, int shared_stream = 1) {
    htm_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_bytes = sizeof(cfg);
    cfg.input_dim = I;
    cfg.column_dim = C;
    cfg.cell_dim = K;
    cfg.active_columns = ACTIVE;
    cfg.enable_sp = cfg.enable_tm = 1;
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
    cfg.use_caller_stream = shared_stream;      // (1 with a NULL stream: the default stream, shared by the members; 0: a stream of its own)
    cfg.shard_world = shard_world;
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (shard_world > 1 && rc != HTM_OK) return nullptr;
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static htm_likelihood_config config(int lp, int es, int hist, int w, int r) {
    htm_likelihood_config c;
    memset(&c, 0, sizeof(c));
    c.struct_bytes = sizeof(c);
    c.learning_period = lp;
    c.estimation_samples = es;
    c.history = hist;
    c.averaging_window = w;
    c.reestimation_period = r;
    return c;
}

static uint64_t bits_of(double x) {
    uint64_t u;
    memcpy(&u, &x, 8);
    return u;
}

static double double_of(uint64_t u) {
    double x;
    memcpy(&x, &u, 8);
    return x;
}

static void arithmetic(const char *path) {
    FILE *f = fopen(path, "r");
    CHECK(f);
    std::vector<double> tail;
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'T') {
            tail.resize(HTM_LIKELIHOOD_TAIL);
            for (double &x : tail) {
                uint64_t u;
                CHECK(fscanf(f, "%" SCNx64, &u) == 1);
                x = double_of(u);
            }
        } else if (kind[0] == 'q') {
            int32_t active, bursting;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNd32, &active, &bursting) == 2);
            printf("%" PRId32 "\n", lik_q_of(active, bursting));
        } else if (kind[0] == 'e') {
            int64_t n, s1, s2;
            CHECK(fscanf(f, "%" SCNd64 " %" SCNd64 " %" SCNd64, &n, &s1, &s2) == 3);
            double mean, std;
            lik_estimate(n, s1, s2, &mean, &std);
            printf("%016" PRIx64 " %016" PRIx64 "\n", bits_of(mean), bits_of(std));
        } else if (kind[0] == 'l') {
            int32_t a;
            uint64_t mean, std;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNx64 " %" SCNx64, &a, &mean, &std) == 3);
            CHECK(tail.size() == HTM_LIKELIHOOD_TAIL);
            printf("%016" PRIx64 "\n", bits_of(lik_likelihood(a, double_of(mean), double_of(std), tail.data())));
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    const int n = 3, words = (I + 31) / 32;
    htm_handle *m[n];
    for (int i = 0; i < n; ++i) m[i] = make_handle(7 + i);
    htm_handle *h = m[0];
    std::vector<double> tail(HTM_LIKELIHOOD_TAIL, 0.25);        // exactly 513: one fewer read is the sanitizer's to report
    const htm_likelihood_config small = config(5, 3, 16, 4, 7);

    // ---- create: refusals, then objects of one and of three streams
    htm_likelihood *lk = nullptr, *one = nullptr, *bad = (htm_likelihood *)1;
    CHECK(htm_likelihood_create(nullptr, &small, tail.data(), n, &lk) == HTM_ERR_ARGUMENT && !lk);
    CHECK(htm_likelihood_create(h, nullptr, tail.data(), n, &lk) == HTM_ERR_ARGUMENT && !lk);
    CHECK(htm_likelihood_create(h, &small, nullptr, n, &lk) == HTM_ERR_ARGUMENT && !lk);
    CHECK(htm_likelihood_create(h, &small, tail.data(), n, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_create(h, &small, tail.data(), 0, &bad) == HTM_ERR_ARGUMENT && !bad);
    CHECK(htm_likelihood_create(h, &small, tail.data(), -2, &lk) == HTM_ERR_ARGUMENT && !lk);
    htm_likelihood_config c = small;
    c.struct_bytes -= 4;
    CHECK(htm_likelihood_create(h, &c, tail.data(), n, &lk) == HTM_ERR_ARGUMENT && !lk);
    const int out_of_range[][5] = {{-1, 3, 16, 4, 7}, {5, 0, 16, 4, 7}, {5, 3, 0, 4, 7}, {5, 3, 16385, 4, 7}, {5, 3, 16, 0, 7}, {5, 3, 16, 65, 7}, {5, 3, 16, 4, 0}};
    for (const auto &p : out_of_range) {
        c = config(p[0], p[1], p[2], p[3], p[4]);
        CHECK(htm_likelihood_create(h, &c, tail.data(), n, &lk) == HTM_ERR_ARGUMENT && !lk);
        CHECK(strlen(htm_last_error(h)) > 0);
    }
    CHECK(htm_likelihood_create(h, &small, tail.data(), n, &lk) == HTM_OK && lk);
    c = config(0, 1, 16384, 64, 1);             // the largest rings
    CHECK(htm_likelihood_create(h, &c, tail.data(), 1, &one) == HTM_OK && one);
    if (htm_handle *sharded = make_handle(3, 2)) {              // a column-sharded handle: HTM_ERR_STATE everywhere
        htm_likelihood *none = nullptr;
        CHECK(htm_likelihood_create(sharded, &small, tail.data(), 1, &none) == HTM_ERR_STATE && !none);
        CHECK(htm_likelihood_reset(lk, sharded, nullptr) == HTM_ERR_STATE);
        htm_destroy(sharded);
    }

    // ---- update: one stream by value, three by the table, launches of at most HTM_LIKELIHOOD_CHUNK steps
    const int T = 2 * HTM_LIKELIHOOD_CHUNK + 3;
    std::vector<htm_step_record> rec_store((size_t)n * T);      // device memory is host memory here; the host code never reads it
    std::vector<double> out_store((size_t)n * T);
    htm_step_record *recs = rec_store.data();
    double *out = out_store.data();
    std::vector<const htm_step_record *> table(n);
    for (int i = 0; i < n; ++i) table[i] = recs + (size_t)i * T;
    CHECK(htm_likelihood_update(lk, h, table.data(), T, out) == HTM_OK);
    CHECK(htm_likelihood_update(lk, h, table.data(), 1, out) == HTM_OK);          // (the same table again)
    std::swap(table[0], table[2]);
    CHECK(htm_likelihood_update(lk, m[1], table.data(), 7, out) == HTM_OK);       // (another table, another handle of the device)
    CHECK(htm_likelihood_update(lk, h, table.data(), 0, out) == HTM_OK);
    CHECK(htm_likelihood_update(one, h, table.data(), T, out) == HTM_OK);
    CHECK(htm_likelihood_update(one, h, table.data(), 0, out) == HTM_OK);
    CHECK(htm_likelihood_update(nullptr, h, table.data(), 1, out) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_update(lk, nullptr, table.data(), 1, out) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_update(lk, h, nullptr, 1, out) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_update(lk, h, table.data(), 1, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_update(lk, h, table.data(), -1, out) == HTM_ERR_ARGUMENT);
    table[1] = nullptr;
    CHECK(htm_likelihood_update(lk, h, table.data(), 1, out) == HTM_ERR_ARGUMENT);
    CHECK(strstr(htm_last_error(h), "stream 1"));
    table[1] = recs + T;

    // ---- reset, export, import
    std::vector<uint8_t> flags = {1, 0, 1};
    CHECK(htm_likelihood_reset(lk, h, flags.data()) == HTM_OK);
    CHECK(htm_likelihood_reset(lk, h, nullptr) == HTM_OK);
    CHECK(htm_likelihood_reset(nullptr, h, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_reset(lk, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    const int64_t bytes = htm_likelihood_state_bytes(lk);
    CHECK(bytes == 3 * 8 * 3 + 16 + 3 * 4 * 4 + 3 * 16 * 4 && htm_likelihood_state_bytes(nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_state_bytes(one) == 8 * 3 + 8 + 64 * 4 + 16384 * 4);
    std::vector<unsigned char> state((size_t)bytes, 0), back((size_t)bytes, 0xff);
    for (size_t i = 3 * 8; i < state.size(); ++i) state[i] = (unsigned char)(i * 7);
    ((int64_t *)state.data())[0] = 5;
    ((int64_t *)state.data())[1] = 0;
    ((int64_t *)state.data())[2] = (int64_t)1 << 40;
    CHECK(htm_likelihood_import(lk, h, state.data(), bytes) == HTM_OK);
    CHECK(htm_likelihood_export(lk, h, back.data(), bytes) == HTM_OK);
    CHECK(state == back);
    CHECK(htm_likelihood_export(lk, h, back.data(), bytes - 8) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_export(lk, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_export(nullptr, h, back.data(), bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_import(lk, h, state.data(), bytes + 8) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_import(lk, h, nullptr, bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_import(lk, nullptr, state.data(), bytes) == HTM_ERR_ARGUMENT);
    ((int64_t *)state.data())[1] = -1;
    CHECK(htm_likelihood_import(lk, h, state.data(), bytes) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_export(lk, h, state.data(), bytes) == HTM_OK && state == back);       // (a refused import changed nothing)

    // ---- scored ticks of a group
    htm_group *g = nullptr;
    CHECK(htm_group_create(m, n, &g) == HTM_OK && g);
    std::vector<uint32_t> packed((size_t)n * words, 0x00010001u);
    std::vector<htm_live_row> rows(n);
    std::vector<int32_t> votes((size_t)n * I);
    std::vector<double> scores(n, -1.0);
    htm_scalar_field fields[1];
    memset(fields, 0, sizeof(fields));
    fields[0].minimum = 0.0; fields[0].scale = 260.0 / 24.0; fields[0].bits = 260; fields[0].width = 21; fields[0].buckets = 260; fields[0].periodic = 1;
    std::vector<double> values(n, 3.5);
    std::vector<int32_t> pairs((size_t)n * 2);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, rows.data(), nullptr, nullptr, lk, scores.data()) == HTM_OK);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), flags.data(), 1, 1, rows.data(), nullptr, votes.data(), lk, scores.data()) == HTM_OK);
    CHECK(htm_likelihood_tick(g, values.data(), fields, 1, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr, lk, scores.data()) == HTM_OK);
    CHECK(htm_likelihood_tick(g, values.data(), fields, 1, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), votes.data(), lk, scores.data()) == HTM_OK);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, nullptr, nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_OK);
    for (int i = 0; i < n; ++i) CHECK(rows[i].capacity_error == 0 && scores[i] == 0.0);      // (the stub's device memory starts as zeros)
    // refusals: one of the pair without the other, an object of another size; the group ticks afterwards
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, lk, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, nullptr, scores.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, one, scores.data()) == HTM_ERR_ARGUMENT);
    CHECK(strstr(htm_group_last_error(g), "streams"));
    CHECK(htm_likelihood_tick(nullptr, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, lk, scores.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, nullptr, nullptr, nullptr, lk, scores.data()) == HTM_ERR_ARGUMENT);
    CHECK(htm_likelihood_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr, lk, scores.data()) == HTM_OK);

    // ---- an object outlives the handles its calls came through: created and updated through one handle, that handle destroyed, then
    // another table through another handle (the object keeps no stream and no staging of the first)
    {
        htm_handle *first = make_handle(31, 1, 0);      // (on a stream of its own, which htm_destroy destroys)
        htm_likelihood *roaming = nullptr;
        CHECK(htm_likelihood_create(first, &small, tail.data(), n, &roaming) == HTM_OK && roaming);
        CHECK(htm_likelihood_update(roaming, first, table.data(), 9, out) == HTM_OK);
        htm_destroy(first);
        std::vector<htm_step_record> other_store((size_t)n * 5);
        std::vector<const htm_step_record *> other(n);
        for (int i = 0; i < n; ++i) other[i] = other_store.data() + (size_t)i * 5;
        CHECK(htm_likelihood_update(roaming, h, other.data(), 5, out) == HTM_OK);
        CHECK(htm_likelihood_reset(roaming, m[1], flags.data()) == HTM_OK);
        CHECK(htm_likelihood_export(roaming, m[2], back.data(), bytes) == HTM_OK);
        htm_likelihood_destroy(roaming);
    }

    // ---- destroy: an object before its handle, one after the group and the handles are gone
    htm_likelihood_destroy(one);
    htm_likelihood_destroy(nullptr);
    htm_group_destroy(g);
    for (int i = 0; i < n; ++i) htm_destroy(m[i]);
    htm_likelihood_destroy(lk);

    if (argc > 1) arithmetic(argv[1]);
    puts("ok");
    return 0;
}
