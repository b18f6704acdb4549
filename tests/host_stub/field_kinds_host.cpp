// The host code of the field kinds under AddressSanitizer + UBSan, as a stand-alone program (tests/test_field_kinds_cpu.py), built
// and linked as tests/host_stub/live_tick_host.cpp is: htm_engine.hip host-only and this file with -fsanitize=address,undefined,
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives the five entry points that take
// a field table -- htm_bank_encode, htm_decode_votes, htm_predicted_value, htm_live_tick, htm_likelihood_tick -- with a mixed
// table of the full sixteen fields and exactly-sized heap buffers, every refusal of the kinds (each must leave the handle and the
// group usable), and, given a case file, evaluates the arithmetic of bithtm_amd/csrc/htm_fields.h on the host:
//     p <seed> <bits> <i>                                         -> pos(i)
//     b <reserved> <buckets> <periodic> <minimum> <scale> <v>     -> bucket(v)       (doubles as 16 hex digits)
// one result per line, then "ok".  Exit status 0 on success.
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"
// the keyed hash and the field arithmetic, as the device compiles them, for the host
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../bithtm_amd/csrc/htm_rng.h"
#include "../../bithtm_amd/csrc/htm_fields.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48;

static htm_handle *make_handle(uint32_t seed) {
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
    cfg.use_caller_stream = 1;                  // (with a NULL stream: the default stream, shared by the members)
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static htm_scalar_field make_field(double minimum, double scale, int offset, int bits, int width, int buckets, int periodic, int reserved) {
    htm_scalar_field f;
    memset(&f, 0, sizeof(f));
    f.minimum = minimum;
    f.scale = scale;
    f.offset = offset;
    f.bits = bits;
    f.width = width;
    f.buckets = buckets;
    f.periodic = periodic;
    f.reserved = reserved;
    return f;
}

// sixteen fields over the 300 bits: a hashed field of width 256 in 40 bits, a category, a periodic and a plain linear field, a
// hashed field of one bit, and eleven more hashed fields of 8 bits with seeds up to 2^29 - 1
static std::vector<htm_scalar_field> sixteen() {
    std::vector<htm_scalar_field> f;
    f.push_back(make_field(0.0, 500.0, 0, 40, 256, 500, 0, HTM_FIELD_HASHED | 5 << 2));
    f.push_back(make_field(0.0, 1.0, 40, 37, 5, 7, 0, HTM_FIELD_CATEGORY));
    f.push_back(make_field(0.0, 2.0, 77, 48, 11, 48, 1, 0));
    f.push_back(make_field(-1.0, 16.5, 125, 37, 5, 33, 0, 0));
    f.push_back(make_field(0.0, 10.0, 162, 1, 3, 10, 0, HTM_FIELD_HASHED | 3 << 2));
    for (int j = 0; j < 11; ++j)
        f.push_back(make_field(0.0, 90.0, 163 + 8 * j, 8, 3, 90, 0, HTM_FIELD_HASHED | (j == 10 ? (1 << 29) - 1 : 9 + j) << 2));
    return f;
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
    char kind[8];
    while (fscanf(f, "%7s", kind) == 1) {
        if (kind[0] == 'p') {
            uint32_t seed, i;
            int32_t bits;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNd32 " %" SCNu32, &seed, &bits, &i) == 3);
            const htm_scalar_field fld = make_field(0.0, 1.0, 0, bits, 1, 1, 0, HTM_FIELD_HASHED | (int32_t)(seed << 2));
            CHECK(field_kind(fld) == HTM_FIELD_HASHED && field_seed(fld) == seed);
            const int pos = field_pos(field_hash_base(fld), i, bits);
            CHECK(pos >= 0 && pos < bits);
            printf("%d\n", pos);
        } else if (kind[0] == 'b') {
            int32_t reserved, buckets, periodic;
            uint64_t minimum, scale, v;
            CHECK(fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNx64 " %" SCNx64 " %" SCNx64, &reserved, &buckets, &periodic, &minimum, &scale, &v) == 6);
            const htm_scalar_field fld = make_field(double_of(minimum), double_of(scale), 0, buckets, 1, buckets, periodic, reserved);
            const int b = field_bucket(fld, double_of(v));
            CHECK(b >= -1 && b < buckets);
            printf("%d\n", b);
        } else {
            CHECK(!"a case kind");
        }
    }
    fclose(f);
}

int main(int argc, char **argv) {
    if (argc > 1) arithmetic(argv[1]);
    CHECK(bits_of(double_of(0x3ff8000000000000ull)) == 0x3ff8000000000000ull);

    const int n = 3, rows_n = 5, words = (I + 31) / 32;
    htm_handle *m[n];
    for (int i = 0; i < n; ++i) m[i] = make_handle(7 + i);
    htm_handle *h = m[0];
    htm_group *g = nullptr;
    CHECK(htm_group_create(m, n, &g) == HTM_OK && g);
    htm_info info;
    CHECK(htm_get_info(h, &info) == HTM_OK);

    const std::vector<htm_scalar_field> tab = sixteen();
    const int F = (int)tab.size();
    CHECK(F == HTM_SCALAR_MAX_FIELDS && tab.back().offset + tab.back().bits <= I);
    CHECK(fields_mixed(tab.data(), F) && !fields_mixed(tab.data() + 2, 2) && field_elements(tab[0]) == 755 && field_elements(tab[1]) == 35 &&
          field_elements(tab[2]) == 48);

    // exactly-sized heap buffers (the stub's device memory is the host heap: the engine's copies are the sanitizer's to check)
    std::vector<double> values((size_t)rows_n * F);
    for (size_t i = 0; i < values.size(); ++i) values[i] = i % 7 == 1 ? NAN : i % 11 == 2 ? INFINITY : i % 13 == 3 ? -1.0 : 0.013 * (double)i;
    std::vector<uint32_t> packed((size_t)rows_n * words, 0u);
    uint32_t *bank = nullptr;
    CHECK(htm_bank_upload(h, packed.data(), rows_n, &bank) == HTM_OK && bank);
    std::vector<int32_t> dvotes((size_t)rows_n * I, 1), dout((size_t)rows_n * F * 2), host_pairs((size_t)F * 2);
    std::vector<htm_live_row> rows(n);
    std::vector<int32_t> pairs((size_t)n * F * 2), votes((size_t)n * I);
    std::vector<double> tick_values((size_t)n * F), scores(n), tail(513, 0.25);     // (htm_likelihood_create's table: exactly 513 doubles)
    for (size_t i = 0; i < tick_values.size(); ++i) tick_values[i] = i % 5 == 4 ? NAN : 0.21 * (double)i;
    std::vector<uint8_t> flags = {1, 0, 1};
    htm_likelihood_config lc;
    memset(&lc, 0, sizeof(lc));
    lc.struct_bytes = sizeof(lc);
    lc.learning_period = 5;
    lc.estimation_samples = 3;
    lc.history = 16;
    lc.averaging_window = 4;
    lc.reestimation_period = 7;
    htm_likelihood *lk = nullptr;
    CHECK(htm_likelihood_create(h, &lc, tail.data(), n, &lk) == HTM_OK && lk);

    // ---- the five entry points over the mixed table
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), rows_n, bank, rows_n, 0) == HTM_OK);
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), 2, bank, rows_n, 3) == HTM_OK);
    CHECK(htm_decode_votes(h, tab.data(), F, dvotes.data(), rows_n, dout.data()) == HTM_OK);
    CHECK(htm_predicted_value(h, tab.data(), F, host_pairs.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 0, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, nullptr, 0, 0, rows.data(), nullptr, nullptr) == HTM_OK);
    CHECK(htm_likelihood_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data(), lk, scores.data()) == HTM_OK);
    // a table of its two linear fields alone, and one field of each other kind alone
    CHECK(htm_live_tick(g, tick_values.data(), tab.data() + 2, 2, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_likelihood_tick(g, tick_values.data(), tab.data(), 1, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr, lk, scores.data()) == HTM_OK);
    CHECK(htm_decode_votes(h, tab.data() + 1, 1, dvotes.data(), rows_n, dout.data()) == HTM_OK);
    for (int i = 0; i < n; ++i) CHECK(rows[i].capacity_error == 0);

    // ---- refusals of the kinds: HTM_ERR_ARGUMENT from every entry point, and everything goes on afterwards
    struct Bad { const char *what; htm_scalar_field f; bool decoding_only; };
    const Bad bad[] = {
        {"reserved < 0", make_field(0.0, 1.0, 0, 40, 5, 36, 0, -1), false},
        {"reserved INT32_MIN", make_field(0.0, 1.0, 0, 40, 5, 36, 0, INT32_MIN), false},
        {"kind 3", make_field(0.0, 1.0, 0, 40, 5, 36, 0, 3), false},
        {"a seed on a linear field", make_field(0.0, 1.0, 0, 40, 5, 36, 0, 4), false},
        {"a seed on a category", make_field(0.0, 1.0, 0, 40, 5, 7, 0, HTM_FIELD_CATEGORY | 4), false},
        {"a periodic category", make_field(0.0, 1.0, 0, 40, 5, 7, 1, HTM_FIELD_CATEGORY), false},
        {"a periodic hashed field", make_field(0.0, 1.0, 0, 40, 5, 70, 1, HTM_FIELD_HASHED), false},
        {"category buckets 0", make_field(0.0, 1.0, 0, 40, 5, 0, 0, HTM_FIELD_CATEGORY), false},
        {"category buckets * width > bits", make_field(0.0, 1.0, 0, 40, 5, 9, 0, HTM_FIELD_CATEGORY), false},
        {"category buckets * width overflows", make_field(0.0, 1.0, 0, 40, 40, INT32_MAX, 0, HTM_FIELD_CATEGORY), false},
        {"hashed buckets 0", make_field(0.0, 1.0, 0, 40, 5, 0, 0, HTM_FIELD_HASHED), false},
        {"hashed buckets INT32_MAX", make_field(0.0, 1.0, 0, 40, 5, INT32_MAX, 0, HTM_FIELD_HASHED), false},
        {"hashed width 257", make_field(0.0, 1.0, 0, 40, HTM_HASHED_MAX_WIDTH + 1, 70, 0, HTM_FIELD_HASHED), false},
        {"hashed buckets + width - 1 = 8193", make_field(0.0, 1.0, 0, 40, 64, HTM_DECODE_MAX_BITS - 62, 0, HTM_FIELD_HASHED), true},
    };
    for (const Bad &b : bad) {
        const htm_scalar_field two[2] = {b.f, tab[3]};
        const int enc = htm_bank_encode(h, two, 2, values.data(), 1, bank, rows_n, 0);
        if (enc != (b.decoding_only ? HTM_OK : HTM_ERR_ARGUMENT)) fprintf(stderr, "%s: htm_bank_encode gave %d\n", b.what, enc);
        CHECK(enc == (b.decoding_only ? HTM_OK : HTM_ERR_ARGUMENT));
        CHECK(htm_decode_votes(h, two, 2, dvotes.data(), 1, dout.data()) == HTM_ERR_ARGUMENT);
        CHECK(strlen(htm_last_error(h)) > 0);
        CHECK(htm_predicted_value(h, two, 2, host_pairs.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_live_tick(g, tick_values.data(), two, 2, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_likelihood_tick(g, tick_values.data(), two, 2, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr, lk, scores.data()) == HTM_ERR_ARGUMENT);
        CHECK(strlen(htm_group_last_error(g)) > 0);
        // (a tick that does not decode takes the field above the decode cap, as htm_bank_encode does)
        CHECK(htm_live_tick(g, tick_values.data(), two, 2, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == (b.decoding_only ? HTM_OK : HTM_ERR_ARGUMENT));
    }
    // the field exactly at the cap decodes
    const htm_scalar_field cap = make_field(0.0, 1.0, 0, 40, 64, HTM_DECODE_MAX_BITS - 63, 0, HTM_FIELD_HASHED | 2 << 2);
    CHECK(field_elements(cap) == HTM_DECODE_MAX_BITS);
    CHECK(htm_decode_votes(h, &cap, 1, dvotes.data(), rows_n, dout.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), &cap, 1, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    // ... and the mixed table still goes through
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), rows_n, bank, rows_n, 0) == HTM_OK);

    htm_likelihood_destroy(lk);
    htm_group_destroy(g);
    for (int i = 0; i < n; ++i) htm_destroy(m[i]);
    puts("ok");
    return 0;
}
