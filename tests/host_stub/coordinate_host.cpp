// The host code of the coordinate fields under AddressSanitizer + UBSan, as a stand-alone program (tests/test_coordinate_cpu.py),
// built and linked as tests/host_stub/field_kinds_host.cpp is: htm_engine.hip host-only and this file with
// -fsanitize=address,undefined, against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the
// engine is bounds-checked on both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives the
// five entry points that take a field table -- htm_bank_encode, htm_decode_votes, htm_predicted_value, htm_live_tick,
// htm_likelihood_tick -- with tables of sixteen entries that end in (and begin with) a coordinate group and exactly-sized heap
// buffers, refusals of the group's layout (each must leave the handle and the group usable), and, given a case file, evaluates
// the arithmetic of bithtm_amd/csrc/htm_coord.h on the host (doubles as 16 hex digits):
//     c <minimum> <scale> <v>                        -> cell(v), or "missing"
//     r <minimum> <scale> <max_radius> <v>           -> radius(v), -1 for a missing one
//     o <seed> <x> <y>                               -> order(x, y)
//     b <seed> <bits> <x> <y>                        -> bit(x, y)
//     s <seed> <width> <cx> <cy> <r>                 -> the winners' candidate indices, ascending, by a plain sort
// one result per line, then "ok".  Exit status 0 on success.
#include <inttypes.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/bithtm_hip.h"
// the keyed hash and the field arithmetic, as the device compiles them, for the host
#define __host__
#define __device__
#define __forceinline__ inline
#include "../../bithtm_amd/csrc/htm_rng.h"
#include "../../bithtm_amd/csrc/htm_fields.h"
#include "../../bithtm_amd/csrc/htm_coord.h"

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

static void push_group(std::vector<htm_scalar_field> &f, int offset, int bits, int width, int max_radius, int seed) {
    f.push_back(make_field(-3.5, 0.25, offset, bits, width, max_radius, 0, HTM_FIELD_COORDINATE | seed << 2));
    f.push_back(make_field(7.0, 4.0, offset, 0, 0, 0, 0, HTM_FIELD_COORDINATE));
    f.push_back(make_field(0.0, 1.0, offset, 0, 0, 0, 0, HTM_FIELD_COORDINATE));
}

// sixteen entries over the 300 bits: a group of width 256 and radius 127 in 40 bits, a hashed field, a category, a periodic and a
// plain linear field, six linear fields of 2 bits, and a group with the largest seed at the table's end
static std::vector<htm_scalar_field> sixteen() {
    std::vector<htm_scalar_field> f;
    push_group(f, 0, 40, 256, 127, 5);
    f.push_back(make_field(0.0, 500.0, 40, 37, 21, 500, 0, HTM_FIELD_HASHED | 5 << 2));
    f.push_back(make_field(0.0, 1.0, 77, 48, 5, 7, 0, HTM_FIELD_CATEGORY));
    f.push_back(make_field(0.0, 2.0, 125, 48, 11, 48, 1, 0));
    f.push_back(make_field(-1.0, 16.5, 173, 37, 5, 33, 0, 0));
    for (int j = 0; j < 6; ++j) f.push_back(make_field(0.0, 1.0, 210 + 2 * j, 2, 1, 2, 0, 0));
    push_group(f, 222, 78, 1, 0, (1 << 29) - 1);
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
        if (kind[0] == 'c') {
            uint64_t minimum, scale, v;
            CHECK(fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx64, &minimum, &scale, &v) == 3);
            const htm_scalar_field fld = make_field(double_of(minimum), double_of(scale), 0, 0, 0, 0, 0, HTM_FIELD_COORDINATE);
            int32_t cell = 0;
            if (coord_cell(fld, double_of(v), &cell)) {
                CHECK(cell >= -(1 << 30) && cell < (1 << 30));
                printf("%d\n", cell);
            } else {
                puts("missing");
            }
        } else if (kind[0] == 'r') {
            uint64_t minimum, scale, v;
            int32_t max_radius;
            CHECK(fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNd32 " %" SCNx64, &minimum, &scale, &max_radius, &v) == 4);
            const htm_scalar_field fld = make_field(double_of(minimum), double_of(scale), 0, 0, 0, 0, 0, HTM_FIELD_COORDINATE);
            const int r = coord_radius(fld, double_of(v), max_radius);
            CHECK(r >= -1 && r <= max_radius);
            printf("%d\n", r);
        } else if (kind[0] == 'o') {
            uint32_t seed;
            int32_t x, y;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNd32 " %" SCNd32, &seed, &x, &y) == 3);
            const uint32_t o = coord_order(coord_order_base(seed), x, y);
            CHECK(o < (1u << 24));
            printf("%u\n", o);
        } else if (kind[0] == 'b') {
            uint32_t seed;
            int32_t bits, x, y;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &seed, &bits, &x, &y) == 4);
            const int b = coord_bit(coord_bit_base(seed), x, y, bits);
            CHECK(b >= 0 && b < bits);
            printf("%d\n", b);
        } else if (kind[0] == 's') {
            uint32_t seed;
            int32_t width, cx, cy, r;
            CHECK(fscanf(f, "%" SCNu32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32, &seed, &width, &cx, &cy, &r) == 5);
            CHECK(r >= 0 && r <= HTM_COORD_MAX_RADIUS && width >= 1);
            const int side = 2 * r + 1, N = side * side;
            const uint32_t base = coord_order_base(seed);
            std::vector<uint32_t> order((size_t)N);
            std::vector<int> index((size_t)N);
            for (int i = 0; i < N; ++i) {
                order[(size_t)i] = coord_order(base, cx - r + i % side, cy - r + i / side);
                index[(size_t)i] = i;
            }
            std::stable_sort(index.begin(), index.end(), [&](int a, int b) { return order[(size_t)a] > order[(size_t)b]; });
            index.resize((size_t)std::min(width, N));
            std::sort(index.begin(), index.end());
            for (size_t i = 0; i < index.size(); ++i) printf(i ? " %d" : "%d", index[i]);
            puts("");
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

    const std::vector<htm_scalar_field> tab = sixteen();
    const int F = (int)tab.size();
    CHECK(F == HTM_SCALAR_MAX_FIELDS && tab.back().offset + tab[F - 3].bits <= I);
    CHECK(fields_coordinate(tab.data(), F) && !fields_coordinate(tab.data() + 3, 10) && fields_mixed(tab.data() + 3, 10) && coord_head(tab[0]) &&
          coord_tail(tab[1]) && coord_tail(tab[2]) && !coord_head(tab[3]) && !coord_tail(tab[3]) && coord_head(tab[13]) && field_seed(tab[13]) == (1u << 29) - 1);

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

    // ---- the five entry points over the table of sixteen
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), rows_n, bank, rows_n, 0) == HTM_OK);
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), 2, bank, rows_n, 3) == HTM_OK);
    CHECK(htm_decode_votes(h, tab.data(), F, dvotes.data(), rows_n, dout.data()) == HTM_OK);
    CHECK(htm_predicted_value(h, tab.data(), F, host_pairs.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 0, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, nullptr, 0, 0, rows.data(), nullptr, nullptr) == HTM_OK);
    CHECK(htm_likelihood_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data(), lk, scores.data()) == HTM_OK);
    // a group alone (the first three entries, the last three), the ten entries between them, and back
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), 3, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_likelihood_tick(g, tick_values.data(), tab.data() + 13, 3, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr, lk, scores.data()) == HTM_OK);
    CHECK(htm_live_tick(g, tick_values.data(), tab.data() + 3, 10, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_decode_votes(h, tab.data() + 13, 3, dvotes.data(), rows_n, dout.data()) == HTM_OK);
    CHECK(htm_bank_encode(h, tab.data(), 3, values.data(), rows_n, bank, rows_n, 0) == HTM_OK);
    for (int i = 0; i < n; ++i) CHECK(rows[i].capacity_error == 0);

    // ---- refusals of the group's layout: HTM_ERR_ARGUMENT from every entry point, and everything goes on afterwards
    const htm_scalar_field head = tab[0], cont = tab[2], linear = tab[6];
    htm_scalar_field wide = head, deep = head, seeded = cont, moved = cont, narrow = head;
    wide.width = HTM_HASHED_MAX_WIDTH + 1;
    deep.buckets = HTM_COORD_MAX_RADIUS + 1;
    seeded.reserved = HTM_FIELD_COORDINATE | 1 << 2;
    moved.offset = 1;
    narrow.width = 0;
    const std::vector<std::vector<htm_scalar_field>> bad = {
        {linear, head}, {linear, head, cont}, {head, linear, cont}, {head, cont, linear}, {cont, linear}, {cont, cont, linear}, {head, cont, cont, cont},
        {wide, cont, cont}, {deep, cont, cont}, {narrow, cont, cont}, {head, seeded, cont}, {head, cont, moved}, {head, cont, head, cont, cont},
    };
    for (const std::vector<htm_scalar_field> &t : bad) {
        const int nf = (int)t.size();
        CHECK(htm_bank_encode(h, t.data(), nf, values.data(), 1, bank, rows_n, 0) == HTM_ERR_ARGUMENT);
        CHECK(htm_decode_votes(h, t.data(), nf, dvotes.data(), 1, dout.data()) == HTM_ERR_ARGUMENT);
        CHECK(strlen(htm_last_error(h)) > 0);
        CHECK(htm_predicted_value(h, t.data(), nf, host_pairs.data()) == HTM_ERR_ARGUMENT);
        CHECK(htm_live_tick(g, tick_values.data(), t.data(), nf, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_ERR_ARGUMENT);
        CHECK(htm_likelihood_tick(g, tick_values.data(), t.data(), nf, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr, lk, scores.data()) == HTM_ERR_ARGUMENT);
        CHECK(strlen(htm_group_last_error(g)) > 0);
    }
    // ... and the table of sixteen still goes through
    CHECK(htm_live_tick(g, tick_values.data(), tab.data(), F, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_bank_encode(h, tab.data(), F, values.data(), rows_n, bank, rows_n, 0) == HTM_OK);

    htm_likelihood_destroy(lk);
    htm_group_destroy(g);
    for (int i = 0; i < n; ++i) htm_destroy(m[i]);
    puts("ok");
    return 0;
}
