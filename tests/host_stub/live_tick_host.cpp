// The host code of the live tick under AddressSanitizer + UBSan, as a stand-alone program (tests/test_live_tick_cpu.py).
// htm_engine.hip is compiled host-only with -fsanitize=address,undefined, this file with the same flags, and both are linked
// against tests/host_stub/hip_stub_runtime.cpp (a HIP runtime made of host memory: every copy of the engine is bounds-checked on
// both sides, kernels do nothing).  The program is run directly; nothing is preloaded.  It drives htm_live_tick and
// htm_live_reset through the C ABI: ticks with a field table and with packed rows, with reset flags and without, with and
// without decoded pairs and votes, every refusal (each must leave the group usable), a group with members on streams of their
// own, a group of inference views, and a group destroyed before and after its members.  Exit status 0 and "ok" on success.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bithtm_hip.h"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                             \
        }                                                                        \
    } while (0)

static const int I = 300, C = 512, K = 48, ACTIVE = 48;

static htm_handle *make_handle(uint32_t seed, int shared_stream) {
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
    cfg.use_caller_stream = shared_stream;      // (1 with a NULL stream: the default stream, shared by the members)
    htm_handle *h = nullptr;
    const int rc = htm_create(&cfg, &h);
    if (rc != HTM_OK) fprintf(stderr, "htm_create: %s\n", htm_last_error(nullptr));
    CHECK(rc == HTM_OK && h);
    return h;
}

static void two_fields(htm_scalar_field *f) {
    memset(f, 0, 2 * sizeof(*f));
    f[0].minimum = 0.0;  f[0].scale = 260.0 / 24.0; f[0].offset = 0;   f[0].bits = 260; f[0].width = 21; f[0].buckets = 260; f[0].periodic = 1;
    f[1].minimum = -1.0; f[1].scale = 33.0 / 2.0;   f[1].offset = 260; f[1].bits = 37;  f[1].width = 5;  f[1].buckets = 33;  f[1].periodic = 0;
}

int main() {
    const int n = 3, words = (I + 31) / 32;
    htm_handle *m[n];
    for (int i = 0; i < n; ++i) m[i] = make_handle(7 + i, 1);
    htm_group *g = nullptr;
    CHECK(htm_group_create(m, n, &g) == HTM_OK && g);

    htm_scalar_field fields[2];
    two_fields(fields);
    // exactly-sized heap buffers: a byte past any of them is the sanitizer's to report
    std::vector<double> values(n * 2);
    for (int i = 0; i < n * 2; ++i) values[i] = i == 1 ? NAN : i == 2 ? INFINITY : 0.5 * i;
    std::vector<uint32_t> packed(n * words, 0x00010001u);
    std::vector<uint8_t> flags = {1, 0, 1};
    std::vector<htm_live_row> rows(n);
    std::vector<int32_t> pairs(n * 2 * 2), votes((size_t)n * I);

    // ticks: values / packed rows, flags / none, every optional output given and not
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, flags.data(), 0, 0, rows.data(), nullptr, nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 0, rows.data(), nullptr, nullptr) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), flags.data(), 1, 1, rows.data(), nullptr, votes.data()) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), flags.data(), 1, 1, rows.data(), nullptr, nullptr) == HTM_OK);
    for (int i = 0; i < n; ++i) CHECK(rows[i].capacity_error == 0);
    CHECK(htm_live_reset(g, flags.data()) == HTM_OK);
    CHECK(htm_live_reset(g, nullptr) == HTM_OK);
    std::vector<uint8_t> none(n, 0);
    CHECK(htm_live_reset(g, none.data()) == HTM_OK);

    // refusals: arguments
    CHECK(htm_live_tick(nullptr, values.data(), fields, 2, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_reset(nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, values.data(), fields, 2, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, values.data(), nullptr, 2, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, values.data(), fields, 0, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, values.data(), fields, 17, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_ERR_ARGUMENT);
    CHECK(htm_live_tick(g, nullptr, fields, 2, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    htm_scalar_field bad[2];
    two_fields(bad);
    bad[1].offset = 270;                            // (reaches past input_dim)
    CHECK(htm_live_tick(g, values.data(), bad, 2, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    two_fields(bad);
    bad[1].offset = 250;                            // (overlaps field 0)
    CHECK(htm_live_tick(g, values.data(), bad, 2, nullptr, nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_ARGUMENT);
    CHECK(strlen(htm_group_last_error(g)) > 0);

    // refusals: the members' state -- parity, reset bits, run feedback, a member that is ahead
    htm_info info;
    CHECK(htm_step(m[1], packed.data(), 1) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_STATE);
    CHECK(strstr(htm_group_last_error(g), "parity"));
    CHECK(htm_live_reset(g, nullptr) == HTM_OK);    // (a reset takes members of either parity)
    CHECK(htm_step(m[0], packed.data(), 1) == HTM_OK && htm_step(m[2], packed.data(), 1) == HTM_OK);
    uint32_t *bank = nullptr;
    CHECK(htm_bank_upload(m[0], packed.data(), n, &bank) == HTM_OK && bank);
    CHECK(htm_set_run_resets(m[2], bank, n) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_STATE);
    CHECK(htm_set_run_resets(m[2], nullptr, 0) == HTM_OK);
    CHECK(htm_set_run_feedback(m[0], bank, n, 1, 0) == HTM_OK);
    CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 0, 1, rows.data(), nullptr, nullptr) < 0);
    CHECK(htm_set_run_feedback(m[0], nullptr, 0, 1, 0) == HTM_OK);
    CHECK(htm_get_info(m[0], &info) == HTM_OK);
    const int64_t before = info.step_index;
    if (htm_run(m[0], bank, n, 4, 1, HTM_RUN_CONTINUE) == HTM_OK && htm_step(m[0], packed.data(), 1) == HTM_ERR_STATE) {   // (ahead now)
        CHECK(htm_live_tick(g, nullptr, nullptr, 0, packed.data(), nullptr, 1, 1, rows.data(), nullptr, nullptr) == HTM_ERR_STATE);
        CHECK(htm_live_reset(g, nullptr) == HTM_ERR_STATE);
        CHECK(htm_live_reset(g, flags.data()) == HTM_ERR_STATE);      // (member 0 is flagged)
    }
    CHECK(htm_run(m[0], bank, n, 2, 1, 0) == HTM_OK);   // (a call without the flag ends the stream)
    CHECK(htm_get_info(m[0], &info) == HTM_OK);
    if ((info.step_index - before) & 1) CHECK(htm_step(m[0], packed.data(), 1) == HTM_OK);
    // ... and the group still ticks
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    // decoding rows of a member's own stay set across a tick
    std::vector<uint32_t> zero_rows((size_t)32 * words, 0);
    uint32_t *own = nullptr;
    CHECK(htm_bank_upload(m[1], zero_rows.data(), 32, &own) == HTM_OK && own);        // (32 rows x W words >= I int32)
    CHECK(htm_set_run_predicted_input(m[1], (int32_t *)own) == HTM_OK);
    CHECK(htm_live_tick(g, values.data(), fields, 2, nullptr, nullptr, 1, 0, rows.data(), pairs.data(), nullptr) == HTM_OK);
    CHECK(htm_set_run_predicted_input(m[1], nullptr) == HTM_OK);

    // inference views: learning refused, learning = 0 ticks with resets
    htm_handle *v[2];
    for (int i = 0; i < 2; ++i) CHECK(htm_create_view(m[0], &v[i]) == HTM_OK && v[i]);
    htm_group *gv = nullptr;
    CHECK(htm_group_create(v, 2, &gv) == HTM_OK && gv);
    CHECK(htm_live_tick(gv, values.data(), fields, 2, nullptr, nullptr, 1, 1, rows.data(), pairs.data(), nullptr) == HTM_ERR_STATE);
    CHECK(htm_live_tick(gv, values.data(), fields, 2, nullptr, flags.data(), 0, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_live_reset(gv, nullptr) == HTM_OK);
    htm_group_destroy(gv);
    for (int i = 0; i < 2; ++i) htm_destroy(v[i]);

    // members on streams of their own; this group is destroyed AFTER its members (it never touches them then)
    htm_handle *p[2] = {make_handle(21, 0), make_handle(22, 0)};
    htm_group *gp = nullptr;
    CHECK(htm_group_create(p, 2, &gp) == HTM_OK && gp);
    CHECK(htm_live_tick(gp, values.data(), fields, 2, nullptr, flags.data(), 1, 1, rows.data(), pairs.data(), votes.data()) == HTM_OK);
    CHECK(htm_live_reset(gp, flags.data()) == HTM_OK);
    for (int i = 0; i < 2; ++i) htm_destroy(p[i]);
    htm_group_destroy(gp);

    htm_group_destroy(g);                           // before its members
    for (int i = 0; i < n; ++i) htm_destroy(m[i]);
    puts("ok");
    return 0;
}
