/*
 * bithtm_hip.h -- C ABI of the MI355X-native bitHTM timestep engine (libbithtm_hip.so).
 *
 * The reference (cokwa/bitHTM) is pure Python/NumPy and has no FFI of its own; its drop-in
 * boundary is the Python class surface bithtm/networks.py:7-149.  This header is the
 * boundary a binding for that surface uses: one handle owns all device state of one
 * SpatialPooler + TemporalMemory pair, one call enqueues one timestep, results are read
 * back lazily.  Plain pointers and sizes only; no C++ or torch types cross it.
 *
 * Every entry point names the reference interface it replaces (file:line relative to the
 * reference checkout).  All functions return 0 on success or a negative htm_status; after
 * a failure htm_last_error() describes it.  A handle is not thread-safe; different
 * handles are independent.  Host buffers are borrowed for the duration of the call only.
 *
 * Cell ids crossing this ABI are the reference's flat ids  col * cell_dim + cell
 * (networks.py:67-71).  Bitmaps are one uint32 word per column, bit j = cell j.
 */
#ifndef BITHTM_HIP_H
#define BITHTM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BITHTM_ABI_VERSION 4

typedef struct htm_handle htm_handle;

typedef enum htm_status {
    HTM_OK = 0,
    HTM_ERR_ARGUMENT = -1,      /* bad pointer / size / field id / config */
    HTM_ERR_HIP = -2,           /* a HIP runtime call failed */
    HTM_ERR_CAPACITY = -3,      /* segment pool or synapse slots exhausted (reported, never silent) */
    HTM_ERR_STATE = -4          /* call not valid in the handle's current state */
} htm_status;

/* Scalars the reference forms implicitly, with the dtype each one ends up in
 * (projections.py:7-11,24,102,205-210; regularizations.py:5-9,16,20-21).  The Python binding
 * computes them with the same Python expressions so they are bit-identical. */
typedef struct htm_config {
    uint32_t struct_bytes;              /* sizeof(htm_config), checked */
    int32_t device;                     /* HIP device ordinal */
    int32_t input_dim;                  /* SpatialPooler.input_dim   (networks.py:18) */
    int32_t column_dim;                 /* column_dim                (networks.py:19,52) */
    int32_t cell_dim;                   /* TemporalMemory.cell_dim   (networks.py:53), 1..64; a column-sharded handle: 1..32 (a model with
                                           still more cells per column keeps its segment store on an engine of ceil(N / 32) columns of
                                           32 cells: DESIGN.md section 7) */
    int32_t active_columns;             /* k                         (networks.py:20,137) */
    int32_t enable_sp;                  /* 0: handle is a stand-alone TemporalMemory */
    int32_t enable_tm;                  /* 0: handle is a stand-alone SpatialPooler */
    /* DenseProjection (projections.py:6-24) */
    double sp_permanence_threshold;     /* permanence >= threshold  <=> connected (:19) */
    double sp_delta_on;                 /* 1.0*(inc+dec)-dec         (:24) */
    double sp_delta_off;                /* 0.0*(inc+dec)-dec         (:24) */
    /* ExponentialBoosting (regularizations.py:4-21) */
    float boost_coefficient;            /* float32(-(intensity/density))  (:16) */
    float duty_momentum;                /* float32(momentum)              (:20) */
    float duty_increment;               /* float32(1.0 - momentum)        (:21) */
    /* PredictiveProjection / SparseProjection (projections.py:97-109,205-293) */
    double tm_learn_active;             /* 1.0*(a-b)+b with a=+increment, b=-decrement (:102,:287) */
    double tm_learn_inactive;           /* 0.0*(a-b)+b */
    double tm_punish_active;            /* same with a=-punishment, b=0.0             (:292) */
    double tm_punish_inactive;
    int32_t tm_learn_prune;             /* min(a,b) < 0 (:105) */
    int32_t tm_punish_prune;
    float tm_permanence_initial;        /* float32(permanence_initial)   (:158) */
    float tm_permanence_threshold;      /* float32(permanence_threshold) (:171) */
    int32_t segment_activation_threshold;   /* (:221) */
    int32_t segment_matching_threshold;     /* (:222) */
    int32_t segment_sampling_synapses;      /* (:223), 1..64 */
    /* fixed-capacity pool replacing DynamicArray2D growth (utils.py:79-135) */
    int32_t segment_capacity;           /* max segment ids (of the whole model); overflow => HTM_ERR_CAPACITY */
    int32_t segment_capacity_local;     /* column-sharded handles: rows for the segments of this rank's own cells
                                           (0 = 2 * segment_capacity / shard_world, at most segment_capacity) */
    int32_t segment_slots;              /* synapse slots per segment, multiple of 64, <= 512 */
    uint32_t seed;                      /* keyed random draws, see bithtm_amd/csrc/htm_rng.h */
    int32_t shard_rank;                 /* column sharding: this handle owns columns               */
    int32_t shard_world;                /*   [rank, rank+1) * column_dim / world; 0 or 1 = unsharded */
    int32_t use_caller_stream;          /* 1: enqueue on `stream` (NULL then means the default stream, e.g.
                                           torch's current stream); 0: create a private stream */
    void *stream;                       /* hipStream_t, see use_caller_stream */
} htm_config;

typedef struct htm_info {
    int64_t step_index;                 /* timesteps processed */
    int32_t segments;                   /* S: allocated segment ids (len(segment_bundle)) */
    int32_t local_segments;             /* rows in use on this handle: = segments, except on a column-sharded handle
                                           (rows of the segments its own cells own, some of them free) */
    int32_t matching_segments;          /* len(distal_state.matching_segment) of the last step */
    int32_t winner_cells;               /* len(winner_cell[0]) of the last step */
    int32_t active_cells;               /* len(active_cell[0]) of the last step */
    int32_t has_distal_state;           /* last_state.distal_state is not None */
    int32_t has_winner_cells;           /* last_state.winner_cell is not None */
    int32_t capacity_error;             /* sticky: 1 = segment pool, 2 = synapse slots, 4 = work list / growth staging,
                                           8 = dead-segment report of a sharded handle, 16 = (internal) a block of the
                                           in-kernel select exchange never arrived: the step's result is invalid, 64 = htm_pack_columns met a
                                           column id outside this handle's input range, 128 = htm_tm_run met a list row with a repeated
                                           column id or one outside [0, column_dim): the results of that call's steps are invalid */
    int32_t words_per_row;              /* packed input words per SP row (input_dim padded to 128 bits) */
    int32_t new_segment_requests;       /* last step: winners without a matching segment (projections.py:271) */
    int32_t recycled_segments;          /* last step: of those, served by recycling (projections.py:80-85) */
    int32_t appended_segments;          /* last step: served by fresh ids (projections.py:90-94) */
    int32_t work_items;                 /* last step: segments that learned or were punished */
    int32_t select_fallbacks;           /* steps so far whose top-k select overflowed the per-block records
                                           and took the exact in-kernel fallback (slower, same result) */
    int32_t candidate_exact_steps;      /* column-sharded handles: steps so far whose LOCAL select cut its threshold bin exactly
                                           instead of handing the whole bin over (slower, same result) */
    int32_t hot_select_steps;           /* column-sharded handles: steps so far whose GLOBAL select was settled among the ranks'
                                           hot lists (the candidates near the previous step's k-th key) without reading the
                                           other candidates */
    int32_t select_zoom_steps;          /* steps so far whose top-k select found its threshold bin crowded (blocks holding several
                                           distinct keys each) and cut it to the k-th key's sub-bin before ranking it */
} htm_info;

/* Device arrays readable with htm_read / writable with htm_write. Element type and count
 * (C = column_dim, k = active_columns, N = C * cell_dim, S = htm_info.segments,
 * E = segment_slots, M = htm_info.matching_segments, Wn = htm_info.winner_cells, W = 32-bit words of cells per column:
 * 1 for cell_dim <= 32, 2 up to 64 -- cell j of column c is bit j % 32 of word c * W + j / 32). */
typedef enum htm_field {
    HTM_F_ACTIVE_COLUMN = 1,   /* int32[k]   State.active_column, ascending (networks.py:29) */
    HTM_F_OVERLAPS = 2,        /* int32[C]   State.overlaps (networks.py:27) */
    HTM_F_BOOSTED = 3,         /* double[C]  State.boosted_overlaps (networks.py:28) */
    HTM_F_DUTY_CYCLE = 4,      /* float[C]   ExponentialBoosting.duty_cycle (regularizations.py:13) */
    HTM_F_CELL_ACTIVATION = 5, /* uint32[C*W] State.cell_activation, packed (networks.py:118-119) */
    HTM_F_CELL_PREDICTION = 6, /* uint32[C*W] State.cell_prediction, packed (networks.py:122) */
    HTM_F_WINNER_WORDS = 7,    /* uint32[C*W] winner cells, packed (networks.py:102) */
    HTM_F_BURSTING = 8,        /* uint8[k]   State.active_column_bursting (networks.py:97) */
    HTM_F_WINNER_CELL = 9,     /* int32[Wn]  flat winner cell ids, ascending (networks.py:103-104) */
    HTM_F_SEG_CELL = 10,       /* int32[S]   segment_bundle (projections.py:226) */
    HTM_F_SEG_NSYN = 11,       /* int32[S]   output_edges (projections.py:42) */
    HTM_F_SEG_PRESYN = 12,     /* int32[S*E] presynaptic flat cell id per slot, -1 = free */
    HTM_F_SEG_PERM = 13,       /* float[S*E] output_permanence (projections.py:44), -1.0 = free */
    HTM_F_SEGCOUNT = 14,       /* int32[N]   bundle_segments (projections.py:227) */
    HTM_F_SEG_POTENTIAL = 15,  /* int32[S]   State.segment_potential (projections.py:246) */
    HTM_F_MATCH_SEGMENT = 16,  /* int32[M]   State.matching_segment, UNORDERED (projections.py:247) */
    HTM_F_MATCH_INFO = 17,     /* uint32[M]  potential | activation<<12 | active<<31, same order */
    HTM_F_MATCH_JITTER = 18,   /* float[M]   matching_segment_jittered_potential, same order */
    HTM_F_CELL_MAX_JITTER = 19,/* float[N]   State.max_jittered_potential (projections.py:236-238) */
    HTM_F_SEG_GID = 20,        /* int32[S]   global segment id of each row: 0..S-1, except on a column-sharded handle,
                                             where the per-segment fields above have htm_info.local_segments rows
                                             (the segments of the rank's own cells; -1 = free row) */
    HTM_F_RECYCLABLE_COUNTS = 21 /* int32[nb + nb2]  READ ONLY (htm_write refuses it): the allocation's counts of recyclable
                                             segments -- rows with fewer synapses than segment_matching_threshold
                                             (projections.py:80-81) -- per 1 024 ids, nb = ceil(S / 1024) of them, then per
                                             2^20 ids, nb2 = ceil(nb / 1024) of them.  For tests and diagnosis: after a
                                             completed step they equal a recount from HTM_F_SEG_NSYN.  HTM_ERR_STATE on a
                                             column-sharded handle, which keeps a dead bit per id instead */
} htm_field;

/* Construction: HierarchicalTemporalMemory.__init__ / SpatialPooler.__init__ /
 * TemporalMemory.__init__ (networks.py:14-24,48-57,132-144).  SP permanences start at zero;
 * upload the matrix drawn as in projections.py:16 with htm_sp_set_permanence. */
int htm_create(const htm_config *config, htm_handle **out);
void htm_destroy(htm_handle *h);
const char *htm_last_error(const htm_handle *h);     /* h may be NULL: error of the last failed htm_create */
int htm_abi_version(void);

/* DenseProjection.permanence (projections.py:16): rows [row_begin, row_begin+row_count) of the
 * float64 [column_dim, input_dim] matrix, row-major, no padding. set rebuilds the connected mask. */
int htm_sp_set_permanence(htm_handle *h, const double *rows, int32_t row_begin, int32_t row_count);

/* TemporalMemory.process(..., epsilon=1e-8) (networks.py:91): the tolerance, compared as float32 the way NumPy compares
 * a Python scalar with float32 arrays, of the "best matching" and "least used" ties (networks.py:81,88) and of the
 * "best matching segment" test of learning (projections.py:267).  0 < epsilon <= 1 (the reference's other uses --
 * prediction > epsilon, max potential < epsilon -- then mean what they mean at 1e-8); stays until set again. */
int htm_set_epsilon(htm_handle *h, float epsilon);
int htm_sp_get_permanence(htm_handle *h, double *rows, int32_t row_begin, int32_t row_count);
/* Unsharded handles with a Spatial Pooler keep a second copy of the connected mask, by byte position ("byte planes": plane j
 * holds byte j of every column's mask row), from which the two-launch schedule of htm_run counts the overlap of an input's
 * non-zero bytes only; an inference view shares its parent's.  Every kernel that writes the mask keeps the planes exact.  This
 * is the check of that: out[0] = the plane bytes that differ from the mask's, compared on the device (0 when all is well; -1 on
 * a handle without planes: a shard), out[1] = the steps so far whose overlap was counted from the planes.  Synchronises. */
int htm_sp_planes_check(htm_handle *h, int64_t out[2]);

/* One timestep, enqueued asynchronously.  packed_input: input bit i is bit (i & 31) of word
 * (i >> 5); ceil(input_dim / 32) host words.
 *   htm_step     HierarchicalTemporalMemory.process(input, learning)   (networks.py:146-149)
 *   htm_sp_step  SpatialPooler.process(input, learning)                (networks.py:26-35)
 *   htm_tm_step  TemporalMemory.process(sp_state, learning=, return_winner_cell=)
 *                (networks.py:91-128) for a stand-alone TM: active_column is a host array of n
 *                distinct column ids (any order; processed in ascending order).
 * htm_step may hold the step's last launch (learning + segment scan) back so that it rides in one of the next htm_step's
 * launches (beside its select finish, or beside its overlap); every other entry point lets it go before doing anything else (htm_sync included), so the only way to observe
 * it is to synchronise the STREAM yourself between two htm_step calls -- call htm_sync instead. */
int htm_step(htm_handle *h, const uint32_t *packed_input, int32_t learning);
int htm_sp_step(htm_handle *h, const uint32_t *packed_input, int32_t learning);
int htm_tm_step(htm_handle *h, const int32_t *active_column, int32_t n, int32_t learning,
                int32_t return_winner_cell);

/* PredictiveProjection.update / .process (projections.py:257-293, :245-255) called on their own -- a caller that writes its
 * own TemporalMemory.process around the device's segment store (its own winner-cell rule, its own punishment mask).
 *   htm_tm_update  learning: columns[i] (distinct, any order, at most active_columns of them) has the learning cells
 *                  winner_words[i] (bit j = cell j: `learning_output` / `output_learning`; cell_dim above 32: two words per listed
 *                  column, side by side, as in the htm_field arrays; bits beyond the column's cells are ignored) -- any number of
 *                  cells per column, up to all of them --, of which unaccounted_words[i] get a new segment (:271-281), bound in
 *                  ascending cell order; punish_words = `output_punishment` as one word (two) per column of the model -- any
 *                  cells, learning cells included --, or NULL = every cell of a column not listed (what TemporalMemory.process
 *                  passes, networks.py:107-108,111).  prev_state, input_activation and winner_input of the reference's
 *                  signature are the handle's previous step (its own last one, or whatever was written with
 *                  htm_import_begin(HTM_IMPORT_PREV_STATE) / htm_write); the previous winners need not be active cells of the
 *                  previous activation, and a segment connected to most of them grows exactly the absent ones.
 *                  On a segment that both learns and is punished the learning update and its growth come first, then the
 *                  punishment (:284-293).
 *                  HTM_ERR_ARGUMENT, nothing enqueued, the handle as it was: n above active_columns, a column listed twice or
 *                  outside [0, column_dim), 65 536 learning cells or more in one call.  HTM_ERR_STATE: a column-sharded handle,
 *                  an inference view.  A pool or a row that ran out sets the sticky capacity flags (htm_get_info).
 *   htm_tm_scan    the scan against the cells of active_words (one word -- two -- per column of the model; bits beyond a
 *                  column's cells are ignored), which become the step's cell activation; closes the timestep.
 *                  PredictiveProjection.State is read with htm_read. */
int htm_tm_update(htm_handle *h, const int32_t *columns, const uint32_t *winner_words, const uint32_t *unaccounted_words,
                  int32_t n, const uint32_t *punish_words);
int htm_tm_scan(htm_handle *h, const uint32_t *active_words);

/* SpatialPooler.process (networks.py:26-35) one phase per call, for handles whose plug-in objects (proximal_projection=,
 * boosting=, inhibition=: networks.py:16,22-24) partly live on the host: the binding interleaves these calls with the
 * user's `process` / `update` methods.  The phases work on the current timestep and do not close it: on a handle with
 * a Temporal Memory htm_tm_step (with the winner list) does, on a Spatial Pooler alone HTM_SP_COMMIT.  Results are
 * read with htm_read (HTM_F_OVERLAPS / _BOOSTED / _ACTIVE_COLUMN).  Each phase is also the stand-alone form of the
 * reference method named beside it. */
typedef enum htm_sp_phase_id {
    HTM_SP_OVERLAP = 1, /* DenseProjection.process (projections.py:18-21) + ExponentialBoosting.process
                           (regularizations.py:15-17); data = packed input as for htm_step */
    HTM_SP_BOOST = 2,   /* ExponentialBoosting.process on overlaps computed elsewhere; data = int32[column_dim], every
                           entry >= 0 (a negative one: HTM_ERR_ARGUMENT, nothing enqueued).  The product float32 factor x
                           overlap is rounded once to double (exact up to 29-bit overlaps) */
    HTM_SP_SELECT = 3,  /* GlobalInhibition.process (regularizations.py:28-29) on the device's boosted overlaps
                           (data = NULL) or on boosted overlaps computed elsewhere (data = double[column_dim]).
                           Accepted data: every finite double >= 0 -- denormals, values up to DBL_MAX, any mix; -0.0
                           counts as 0.  The result is exactly the active_columns largest, lower column first among
                           equal values, over all 64 bits of each value (also after HTM_SP_BOOST: the select of values
                           that came from the host launches every radix digit and assumes nothing about their width).
                           NaN, +-inf or a negative value: HTM_ERR_ARGUMENT with a message naming the column, nothing
                           enqueued, the handle stays usable.  HTM_F_BOOSTED reads back the caller's own values */
    HTM_SP_ACTIVE = 4,  /* a winner list chosen elsewhere; data = int32[count] distinct columns, count <= active_columns */
    HTM_SP_LEARN = 5,   /* DenseProjection.update (projections.py:23-24) on the current winner list; data = packed
                           input, or NULL: the input of HTM_SP_OVERLAP */
    HTM_SP_DUTY = 6,    /* ExponentialBoosting.update (regularizations.py:19-21) on the current winner list */
    HTM_SP_COMMIT = 7   /* close the timestep of a handle without Temporal Memory */
} htm_sp_phase_id;
int htm_sp_phase(htm_handle *h, int32_t phase, const void *data, int64_t count);

/* n_steps timesteps of htm_step over a bank of n_inputs packed inputs that is ALREADY IN
 * DEVICE MEMORY (words_per_row words each, see htm_info); step t reads input
 * (step_index % n_inputs).  Nothing is copied or synchronised: this is the loop
 * example.py:48-53 runs, with the input bank resident in HBM.  use_graph bit 0: replay captured
 * hipGraphs (one per step, or per 16 steady-state steps) instead of issuing the launches one by one;
 * bit 1: do NOT pipeline.  By default the Spatial Pooler works ahead of the Temporal Memory inside the
 * call -- the next step's overlaps and winner list are computed in the two launches of the current TM step
 * (its permanence and duty-cycle updates are not ahead; in the four-launch schedule a handle falls back to when the
 * scan's column bitmap does not fit the LDS they are) --; it never looks past n_steps, so the state a call leaves
 * behind is exactly that of n_steps htm_step calls. */
int htm_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps,
            int32_t learning, int32_t use_graph);
/* use_graph bit 2 (HTM_RUN_CONTINUE): a caller that streams its input in chunks promises that the next call is another
 * htm_run on the same bank, n_inputs and learning flag.  The Spatial Pooler then keeps working ahead across the end
 * of this call (the next step's overlaps and winner list are computed beside this call's last Temporal Memory
 * step) and the next call starts in the steady state instead of with a cold start of three more launches.  Until a
 * later htm_run ends without the bit, every other call that needs the Spatial Pooler's state (htm_step, htm_sp_*,
 * htm_tm_step, state import, the Spatial Pooler fields of htm_read) returns HTM_ERR_STATE; the Temporal Memory's state
 * is that of exactly the steps run so far.  Where the pipelined schedule is not available the bit is ignored; a handle
 * that is ahead when the schedule becomes unavailable (another handle with its own stream appears on the device)
 * finishes the step it had begun in the schedule it began it in and goes on unpipelined -- never an error. */
#define HTM_RUN_GRAPH 1
#define HTM_RUN_NO_PIPELINE 2
#define HTM_RUN_CONTINUE 4

/* Capture and instantiate, without running anything, every hipGraph the htm_run call with the same
 * arguments will replay when it comes next (graphs are otherwise built lazily inside htm_run, the first
 * time a launch pattern is met).  Latency-sensitive callers invoke it once after their warm-up. */
int htm_prepare(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps,
                int32_t learning, int32_t use_graph);

/* What an htm_run / htm_prepare call with these arguments would do if it came now (nothing is enqueued): a caller that
 * reports how it ran (bench.py's `config.hip_graph`) asks instead of assuming.  Bits of the result:
 *   HTM_PLAN_GRAPH      the steady-state steps replay hipGraphs (use_graph bit 0 AND n_steps at or above the eager limit,
 *                       64 unless BITHTM_EAGER_BELOW says otherwise, AND no htm_profile collection in progress)
 *   HTM_PLAN_PIPELINED  the Spatial Pooler works ahead of the Temporal Memory (heterogeneous launches)
 *   HTM_PLAN_LEAN       ... in the two-launch schedule (three under BITHTM_LEAN=1; else four launches per step)
 *   HTM_PLAN_SCAN_LARGE the segment scan runs in its streaming (large-pool) form
 * Negative: an error status. */
#define HTM_PLAN_GRAPH 1
#define HTM_PLAN_PIPELINED 2
#define HTM_PLAN_LEAN 4
#define HTM_PLAN_SCAN_LARGE 8
int htm_run_plan(htm_handle *h, int32_t n_steps, int32_t use_graph);

/* htm_run with a per-step record, written on the device and read back by the caller once per call (the per-step report of
 * example.py:55-57 without a State read-back per step).  Record i belongs to the i-th step of THIS call; "the state before"
 * a step is the reference's last_state before its process() call (for a fresh handle: no predictions).
 *   htm_step_record      eight int32 counts per step, in reference terms:
 *     active_columns            len(sp_state.active_column)
 *     bursting_columns          tm_state.active_column_bursting.sum()                      (networks.py:97)
 *     predicted_columns_before  last_state.cell_prediction.any(axis=1).sum() of the state before the step
 *     predicted_columns         the same for this step's cell_prediction                   (networks.py:122)
 *     active_cells              len(tm_state.active_cell[0])
 *     winner_cells              len(tm_state.winner_cell[0])
 *     segments                  htm_info.segments after the step
 *     new_segments              htm_info.recycled_segments + appended_segments of the step
 *   htm_run_record       struct_bytes = sizeof(htm_run_record), then DEVICE pointers, NULL = not requested (at least one set):
 *     records                   htm_step_record[n_steps]
 *     active_column             int32[n_steps * k]: sp_state.active_column of each step, ascending
 *     column_prediction         uint32[n_steps * ceil(C / 32)]: bit c of a step's words = cell_prediction[c].any()
 * Buffer sizes are the caller's contract, as for htm_run's bank.  rec == NULL: exactly htm_run.  All use_graph bits keep their
 * meaning; the records of a continuing call (HTM_RUN_CONTINUE) hold its own steps only, never the step the Spatial Pooler has
 * begun ahead.  The graphs of recorded steps are captured once (htm_prepare_recorded builds them ahead, as htm_prepare does
 * for htm_run) and read the buffers from a descriptor the call fills on the device: another call with other buffers
 * replays the same graphs.  A column-sharded handle, or column_dim of 2^24 or more: HTM_ERR_STATE; a wrong struct_bytes or no
 * buffer: HTM_ERR_ARGUMENT. */
typedef struct htm_step_record {
    int32_t active_columns;
    int32_t bursting_columns;
    int32_t predicted_columns_before;
    int32_t predicted_columns;
    int32_t active_cells;
    int32_t winner_cells;
    int32_t segments;
    int32_t new_segments;
} htm_step_record;

typedef struct htm_run_record {
    uint32_t struct_bytes;              /* sizeof(htm_run_record), checked */
    htm_step_record *records;           /* device, [n_steps], or NULL */
    int32_t *active_column;             /* device, [n_steps * active_columns], or NULL */
    uint32_t *column_prediction;        /* device, [n_steps * ceil(column_dim / 32)], or NULL */
} htm_run_record;

int htm_run_recorded(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning,
                     int32_t use_graph, const htm_run_record *rec);
int htm_prepare_recorded(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning,
                         int32_t use_graph);
/* Sequence resets.  A reset before step t makes step t run as the reference does after
 * `tm.last_state = tm.get_empty_state()` (networks.py:57-65,91-93): the state before it has no predictions, so every active
 * column bursts; distal_state is None, so there are no best-matching cells (winners are the least-used cells, keyed draw
 * stream 1 as usual) and no distal_projection.update -- no reinforcement, punishment, growth or new segments in step t
 * (projections.py:257-259); winner_cell is None.  The segment store, the Spatial Pooler, the step index (so the keyed draws
 * of later steps are those of a run without the reset), epsilon and the sticky capacity flags stay what they are.  In a
 * recorded run a reset step's "state before" is that empty state: predicted_columns_before = 0.
 *
 * htm_reset: the handle's previous step becomes that empty state, on the device (one launch on the handle's stream, no host
 * copy, no wait) -- what htm_import_begin(HTM_IMPORT_PREV_STATE) + htm_write of get_empty_state()'s fields + htm_import_commit
 * leave, and what htm_read then returns.  For htm_step, htm_tm_step and htm_sp_phase / htm_tm_update / htm_tm_scan callers
 * alike, between two steps.  HTM_ERR_STATE while the handle is ahead (HTM_RUN_CONTINUE), while a step opened with
 * htm_shard_begin is not finished, on a column-sharded handle and on a handle without a Temporal Memory.
 *
 * htm_set_run_resets: reset bits of the later htm_run / htm_run_recorded / htm_prepare / htm_prepare_recorded calls on banks of
 * n_inputs rows.  device_bits: DEVICE words, 32 bits each, bit r of word r / 32 = reset before every step that reads bank
 * row r (step t reads row t % n_inputs), so the bits cycle with the bank across epochs and HTM_RUN_CONTINUE calls.  The
 * words are read by the run while it executes: they must stay valid, as the bank must.  NULL clears the bits (runs then
 * launch and capture exactly what they did without them).  A run on a bank of another n_inputs while bits are set:
 * HTM_ERR_ARGUMENT.  The graphs of runs with resets are captured once and read the bits through a descriptor the call fills
 * on the device: a call with other bits replays the same graphs.  A column-sharded handle: HTM_ERR_STATE. */
int htm_reset(htm_handle *h);
int htm_set_run_resets(htm_handle *h, const uint32_t *device_bits, int32_t n_inputs);
/* Predicted-input decoding: which input the state expects next, as the top-down pass of the Spatial Pooler's proximal
 * projection over the predicted columns.  The votes of a state are int32[input_dim]:
 *   votes[i] = number of columns c with a predicted cell (cell_prediction.any(axis=1), networks.py:30-33,122) whose
 *              connection to input i is connected (permanence[c, i] >= permanence_threshold, projections.py:18-21)
 * -- the reference's (pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0) with
 * pp = spatial_pooler.proximal_projection, right after the step that left the state.  The prediction is the one step t makes
 * about step t + 1, and the mask is the one after step t's Spatial Pooler update: the one step t + 1's overlap reads, so
 * votes_t . x_{t+1} = the sum of step t+1's overlaps over the columns step t predicts.  A state without predictions (a fresh
 * handle, a reset) gives zeros.
 *
 * htm_predicted_input: the votes of the handle's current state (after htm_step, htm_run, a group call, htm_reset or an
 * import) into host_dst[input_dim]: after the held-back tail, one launch and a synchronising copy, as htm_read.
 * HTM_ERR_STATE while the handle is ahead (HTM_RUN_CONTINUE), while a step opened with htm_shard_begin or htm_sp_phase is not
 * finished, on a column-sharded handle and on a handle without the device's own Spatial Pooler and Temporal Memory.
 *
 * htm_set_run_predicted_input: DEVICE rows of votes for the later htm_run / htm_run_recorded calls, and for the htm_group_run /
 * htm_group_step calls of groups the handle is a member of: such a call of n_steps steps writes n_steps x input_dim int32,
 * the votes of the state its step i leaves in row i (taken behind that step, so a reset before the next step does not change
 * them).  The rows must stay valid while the call executes.  htm_prepare / htm_prepare_recorded capture the graphs of such
 * calls.  NULL clears the rows (calls then launch and capture exactly what they did without them).  The graphs of decoding
 * calls are captured once and read the rows through a descriptor the call fills on the device.  Where the handle's run would
 * take the four-launch pipelined schedule (it applies the Spatial Pooler's rows of step t + 1 before step t's predictions
 * exist), decoding calls run unpipelined, and htm_run_plan reports them so.  HTM_ERR_STATE on a column-sharded handle and on a
 * handle without the device's own Spatial Pooler and Temporal Memory. */
int htm_predicted_input(htm_handle *h, int32_t *host_dst);
int htm_set_run_predicted_input(htm_handle *h, int32_t *device_votes);

/* hipGraphs the handle holds (captured and instantiated by htm_run / htm_prepare / htm_shard_run / htm_tm_run / htm_sp_run and their recorded forms);
 * diagnostic: a recorded call with other buffers replays the graphs of the one before and adds none. */
int htm_graph_count(htm_handle *h);

/* Convenience for callers without their own device allocator: copy n_inputs packed inputs
 * (ceil(input_dim/32) host words each, as for htm_step) into a handle-owned device bank laid out
 * as htm_run expects, and return its device address.  Freed by htm_destroy. */
int htm_bank_upload(htm_handle *h, const uint32_t *host_inputs, int32_t n_inputs, uint32_t **device_bank);

/* Column-sharded timestep (one handle per GPU, shard_world > 1; DESIGN.md "Multi-GPU").  The
 * reference has no counterpart: it is HierarchicalTemporalMemory.process (networks.py:146-149)
 * split around the one exchange the sharding needs.
 *   htm_shard_begin   the rank's own part that precedes the exchange; writes this rank's record
 *                     (htm_shard_record_bytes bytes) to send_device.  The input is either a
 *                     device bank as for htm_run (packed_input == NULL) or one host input as for
 *                     htm_step (device_inputs == NULL).
 *   (caller)          all-gather of the records in rank order into recv_device
 *                     (world * record bytes) on the same stream, e.g. RCCL ncclAllGather
 *   htm_shard_finish  global top-k, segment allocation and this rank's share of the learning and
 *                     of the segment scan.
 * With identical inputs on all ranks the union of the ranks' results equals the unsharded result
 * bit for bit. */
int64_t htm_shard_record_bytes(htm_handle *h);
int htm_shard_begin(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, const uint32_t *packed_input,
                    int32_t learning, void *send_device);
int htm_shard_finish(htm_handle *h, const void *recv_device, int32_t learning);

/* The same timestep as ONE call, with the exchange done inside the library by RCCL (ncclAllGather on the
 * handle's stream, device to device over xGMI; librccl is loaded when first needed).  One process per GPU:
 *   rank 0:     htm_shard_unique_id(id)          128 bytes, handed to the other ranks by the caller
 *   every rank: htm_shard_comm_init(h, id)       collective (ncclCommInitRank); allocates the record buffers
 *   every rank: htm_shard_step(h, ...)           per timestep; the input as for htm_shard_begin */
int htm_shard_unique_id(void *out128);
int htm_shard_comm_init(htm_handle *h, const void *unique_id128);
int htm_shard_step(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, const uint32_t *packed_input,
                   int32_t learning);
int htm_shard_comm_size(htm_handle *h);              /* ranks of that communicator (ncclCommCount), or a negative status */
int htm_shard_graph_ok(htm_handle *h);               /* 1: htm_shard_comm_init's preflight (a record-sized all-gather over this
                                                        communicator, checked, then captured into a hipGraph, replayed and checked
                                                        again) passed and htm_shard_run replays graphs; 0: it launches eagerly */
/* n_steps of htm_shard_step over a bank resident in device memory, without the host in the loop: the launches of whole
 * timesteps, the collective included, are replayed as hipGraphs (use_graph bit 0; RCCL's all-gather is captured like a
 * kernel -- where the runtime refuses, the call launches eagerly instead), and inside the call the overlap of step t + 1 on
 * the rank's own columns rides in the last launch of step t (bit 1, HTM_RUN_NO_PIPELINE: not).  The state a call leaves
 * behind is that of n_steps htm_shard_step calls.  htm_shard_group_run: the same for all the ranks of a group inside one
 * process (see htm_shard_group_step). */
int htm_shard_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning, int32_t use_graph);
int htm_shard_group_run(htm_handle *const *handles, int32_t n, const uint32_t *const *device_inputs, int32_t n_inputs, int32_t n_steps,
                        int32_t learning, int32_t use_graph);
/* RCCL round trip at world size 1 on `device` (communicator, all-gather on a stream, compare; then the same collective
 * captured into a hipGraph and replayed): what a box with one GPU can verify of the path htm_shard_step / htm_shard_run
 * take.  0: both work; 1: the collective works but is not capturable on this runtime; negative: failure. */
int htm_rccl_selftest(int32_t device);

/* The keyed random draws of the engine (bithtm_amd/csrc/htm_rng.h), computed on the host: out[i] =
 * the number in [0, 1) -- a multiple of 2^-24 -- that the step `step` of a handle created with `seed` uses for
 *   stream 1  the least-used-cell jitter of flat cell a[i]                                     (networks.py:87)
 *   stream 2  the growth priority of presynaptic cell b[i] for segment a[i]                    (projections.py:120)
 *   stream 3  the jitter of matching segment a[i]                                              (projections.py:235)
 * (b may be NULL: all zeros).  This is the direction in which the reference and the engine are made to agree draw for
 * draw: the reference consumes THESE numbers where it would call np.random.rand (INTEGRATION.md section 5 shows the patch);
 * the engine cannot take MT19937's instead -- their shapes depend on data the step has not produced yet when it starts. */
int htm_keyed_draws(uint32_t seed, int32_t stream, uint32_t step, const uint32_t *a, const uint32_t *b, int64_t n, double *out);

/* All the shards of one model inside ONE process on one device: handles[r] = rank r of n = shard_world, created on
 * the same stream; the all-gather becomes n x n device copies.  For tests and single-GPU rehearsals of the sharded
 * path.  device_inputs[r] = rank r's copy of the input bank (or NULL and one host input, as for htm_step). */
int htm_shard_group_step(htm_handle *const *handles, int32_t n, const uint32_t *const *device_inputs, int32_t n_inputs,
                         const uint32_t *packed_input, int32_t learning);

/* Pre-populated segment pool, generated on the device (BASELINE.json configs[4]: 255 segments per cell, a pure
 * scan stress): every cell with flat id in [cell_begin, cell_end) gets segments_per_cell segments of `synapses`
 * synapses (>= the matching threshold, <= 64) to keyed-random distinct presynaptic cells with permanences keyed-
 * uniform in [perm_lo, perm_hi); segment ids are (cell - cell_begin) * segments_per_cell + j.  Fresh handles only.
 * On a column-sharded handle only the rows of its own cells are generated; give every handle of the group the
 * same range.  (The reference grows its store step by step, projections.py:226; it has no counterpart.) */
int htm_populate(htm_handle *h, int64_t cell_begin, int64_t cell_end, int32_t segments_per_cell, int32_t synapses,
                 double perm_lo, double perm_hi, uint32_t seed);

int htm_sync(htm_handle *h);
/* the hipStream_t the handle enqueues on (its own, or the caller's: htm_config.use_caller_stream) -- for callers that order
 * their own work against it, and for creating further handles on the same stream */
int htm_get_stream(htm_handle *h, void **stream);
int htm_get_info(htm_handle *h, htm_info *out);      /* synchronises; HTM_ERR_CAPACITY (with *out filled
                                                         in) once a fixed-capacity pool has overflowed */

/* Lazy read-back of State fields / state export (synchronises); count = number of ELEMENTS
 * the caller's buffer holds; it must be >= the field's current element count. Returns the
 * number of elements written (>= 0) or a negative status. */
int64_t htm_read(htm_handle *h, int32_t field, void *dst, int64_t count);

/* Rows [row_begin, row_begin + row_count) of a per-segment field (HTM_F_SEG_CELL / _NSYN / _PRESYN / _PERM / _POTENTIAL /
 * _GID, same element types as htm_read), for pools too large to read whole (the reference's `segment_bundle[a:b]`,
 * `output_edge[a:b]`, `output_permanence[a:b]`: projections.py:226,43-44).  HTM_F_MATCH_INFO comes back DENSE here: one
 * word per row, potential | activation<<12 | active<<31 for a matching row, 0 otherwise.  count = elements dst holds. */
int64_t htm_read_rows(htm_handle *h, int32_t field, int64_t row_begin, int64_t row_count, void *dst, int64_t count);

/* State import (checkpoint / hand-off from another implementation), in three steps:
 *   htm_import_begin(h, step_index)   the state being imported is "after step_index steps"
 *   htm_write(h, field, src, count)   the arrays of htm_read, same element types
 *   htm_import_commit(...)            the scalars that go with them; rebuilds derived state
 * SP permanences are imported with htm_sp_set_permanence.
 * htm_import_begin(h, HTM_IMPORT_PREV_STATE): TemporalMemory.process(..., prev_state=X) (networks.py:92-93) -- only the
 * fields of the previous step's State are written (cell words, winner cells, MATCH_* / SEG_POTENTIAL / CELL_MAX_JITTER);
 * the segment store, the step index and the sticky capacity flags stay what they are (`segments` of the commit is ignored). */
#define HTM_IMPORT_PREV_STATE (-1)
int htm_import_begin(htm_handle *h, int64_t step_index);
int htm_write(htm_handle *h, int32_t field, const void *src, int64_t count);
int htm_import_commit(htm_handle *h, int32_t segments, int32_t matching_segments, int32_t winner_cells,
                      int32_t has_distal_state, int32_t has_winner_cells);

/* Per-kernel device time of the most recent htm_run: names[i] / total_ms[i] / launches[i] for
 * up to max_kernels kernels (HIP events on the handle's stream).  Only collected when
 * htm_profile(h, 1) was called before the run (profiled runs are slower). */
int htm_profile(htm_handle *h, int32_t enable);
int htm_profile_read(htm_handle *h, int32_t max_kernels, const char **names, double *total_ms,
                     int64_t *launches);

/* Device-clock timeline of the pipelined launches (diagnostic; handle created with the environment
 * variable BITHTM_TRACE=1, otherwise HTM_ERR_STATE).  dst receives 8 x 4096 x 2 values: for slot =
 * launch (0..2; 0..3 in the four-launch schedule) + 4 * step parity and block b, the 100 MHz device wall clock when the block
 * started and when it ended, 0 where that block did not run.  Each launch overwrites its slot,
 * so after a run the buffer holds the last two steps -- of those with an index below BITHTM_TRACE_UNTIL,
 * if that is set (the last step of a run looks ahead less than the steady state).  Returns the
 * number of values. */
#define HTM_TRACE_VALUES (8 * 4096 * 2)
int64_t htm_trace_read(htm_handle *h, uint64_t *dst, int64_t count);

/* Model groups: n independent models of one shape stepped together.  Every launch of a group step
 * covers all members (grid y = member), each member on its own device state; every member ends bit-identical to the same
 * model stepped alone by htm_run / htm_run_recorded / htm_step.
 *
 * htm_group_create: members are unsharded handles with SP and TM on one device, pairwise distinct, with equal input_dim,
 * column_dim, cell_dim (<= 64), active_columns, segment_capacity and segment_slots; seeds, the scalar learning parameters and
 * the learned state may differ.  A member that is ahead (HTM_RUN_CONTINUE) or has open phases (htm_sp_phase): HTM_ERR_STATE.
 * Nothing is enqueued before an error returns.  The group keeps the member pointers: destroy it before any of its members.
 *
 * htm_group_run: n_steps steps of every member; member i reads row (its step index) % n_inputs of device_banks[i] (each bank
 * as htm_run's).  All members must have the same step parity (HTM_ERR_STATE otherwise).  records: NULL, or n htm_run_record
 * (one per member, as htm_run_recorded's).  use_graph bit 0: replay hipGraphs of the group's steps (one stream, no forked
 * branches; calls of fewer than BITHTM_EAGER_BELOW steps launch eagerly).  The group enqueues on the first member's stream;
 * for a member on another stream the host waits for that stream before the call and for the group's stream at its end
 * (hipStreamSynchronize, outside any capture).  As htm_run does, the end of a call copies each member's segment count into
 * the member's pinned hint word (no wait) for its next call's scan.  Capacity overflows set the sticky
 * flags of the member that overflowed (htm_get_info of that member).  Sequence resets inside a group run are not available:
 * a member with reset bits set (htm_set_run_resets) is refused.
 *
 * htm_group_step: one step of every member on host inputs: packed_inputs holds n rows of ceil(input_dim / 32) words, row i
 * for member i (copied into a group-owned staging bank).  records as for htm_group_run, one step each.
 *
 * Both write the predicted-input votes of every member that has decoding rows set (htm_set_run_predicted_input) into those
 * rows, step i of the call in row i, one launch per step for all members (a group applies each step's Spatial Pooler rows
 * within that step).
 *
 * Afterwards every per-member call works as after htm_run: htm_read, htm_get_info, htm_step, htm_run, export / import. */
typedef struct htm_group htm_group;
int htm_group_create(htm_handle *const *members, int32_t n, htm_group **out);
void htm_group_destroy(htm_group *g);
const char *htm_group_last_error(const htm_group *g);
int htm_group_run(htm_group *g, const uint32_t *const *device_banks, int32_t n_inputs, int32_t n_steps, int32_t learning,
                  int32_t use_graph, const htm_run_record *records);
int htm_group_step(htm_group *g, const uint32_t *packed_inputs, int32_t learning, const htm_run_record *records);

/* Inference views: many input streams stepped over ONE copy of a trained model's weights.
 *
 * htm_create_view: a new handle whose device state ALIASES the parent's weights -- the Spatial Pooler's permanences and
 * connected mask, the segment store (owner cells, synapse counts, presynaptic cells, permanences, segments per cell) -- and
 * OWNS its stream state: duty cycles, overlaps and select state, cell words, winner list, the last scan's matching segments and
 * per-cell maxima, the counter block, the record / reset / decoding descriptors.  The view starts as its parent would be right
 * after htm_reset: same duty cycles, step index, seed, epsilon and configuration; empty Temporal Memory state.  Stepping a view
 * (learning = 0 only) therefore equals stepping a full copy of the parent (export + import) after htm_reset with learning = 0.
 * The parent must be unsharded, with SP and TM, not a view itself and not ahead (HTM_RUN_CONTINUE): HTM_ERR_STATE otherwise.
 *
 * Lifetime: the weights (and the parent's own stream, if it created one) are reference-counted: freed when the last of the
 * parent and its views is destroyed, in any order of the htm_destroy calls.
 *
 * Ordering: a view enqueues on its parent's stream.  Every stepping call on a view (htm_step, htm_run*, htm_prepare*,
 * htm_reset, htm_predicted_input, htm_tm_step, htm_tm_scan, group calls with view members) first lets the parent's held-back
 * launch go, refuses with HTM_ERR_STATE while the parent is ahead (HTM_RUN_CONTINUE), and copies the parent's segment count
 * into the view's counter block (a device-to-device copy on the shared stream).  A view thus always sees the parent's current
 * weights; the parent may keep learning between view calls.  A view holds no launch back across calls.
 *
 * Refused on a view (HTM_ERR_STATE, nothing enqueued): learning != 0; writes of weight fields (htm_write of SEG_* / SEGCOUNT,
 * htm_sp_set_permanence, htm_populate, htm_tm_update, htm_sp_phase); state import other than HTM_IMPORT_PREV_STATE; the shard
 * entry points; a view of a view.
 *
 * htm_device_bytes: the device bytes this handle allocated itself (a view does not count the weights it aliases), or
 * HTM_ERR_ARGUMENT for NULL.
 *
 * Groups take view members as any others.  A group call with learning != 0 and a view member is refused.  With the environment
 * knob BITHTM_SHARED_SCAN=1 (read when the group's first member is created), a group whose members all alias one set of weights
 * (views of one parent, with or without the parent) and that has a view member scans the store ONCE per step for up to M
 * members at a time (kgrp_scan_shared: M member bitmaps in LDS, at most 64 KiB; BITHTM_SHARED_SCAN_MEMBERS caps M),
 * bit-identical to the per-member scan.  It is off by default: it reads fewer bytes but measured slower. */
int htm_create_view(htm_handle *parent, htm_handle **out);
int64_t htm_device_bytes(htm_handle *h);

/* Stream forks: a view that continues ANOTHER handle's stream.
 *
 * htm_view_sync: the stream state of `view` (an inference view, htm_create_view) becomes that of `source` -- its parent, or another
 * view of the same parent -- as `source` is after the calls made on it so far.  One launch on the shared stream (after the held-
 * back launch of the source and of the parent); no copy through the host, no wait: the per-segment arrays are bounded by the
 * source's segment count as the DEVICE holds it.  What comes over: the duty cycles, the step index and its parity; the previous
 * step's prediction, activation and winner words, its winner list and active-column list; the column bitmaps, ranks and
 * bursting flags; overlaps, boosted overlaps and the select's state; the matching segments of the last scan (info words, jitter,
 * match bits of both parities -- rows of the view at and above the source's count read "not matching" afterwards) and the
 * per-cell maxima; n_win, has_winner, has_distal, cm_dense_step and the rest of the counter block, except that the learning
 * role's counts and the sticky capacity flags start clean, as in htm_create_view.  The host's part of the stream comes over too
 * (step index, the lower bound of the segment count, whether a select window is known).  Stepping the view from here equals
 * stepping a full copy of the source (export + import, WITHOUT htm_reset) with learning = 0, bit for bit.  The source is not
 * changed.  The per-cell maxima the view receives are as current with the weights as the source's: the view's next call does
 * not wait for the stream (as a view's first call after its parent learned otherwise does).
 * HTM_ERR_ARGUMENT: a NULL handle (nothing is touched).  HTM_ERR_STATE, nothing enqueued: `view` is not a view; the handles do not
 * share weights; view == source; either handle has a step open (htm_sp_phase); the view, the source or the parent is ahead
 * (HTM_RUN_CONTINUE).
 *
 * htm_bank_rows: device_dst row r = row (first_step + r) % bank_rows of device_bank, r in [0, n): the rows a run of n steps from
 * step index first_step read -- or, with htm_set_run_feedback, the forecast rows it left -- made contiguous.  One launch on the
 * handle's stream; no wait.  Rows are words_per_row words.  HTM_ERR_ARGUMENT: NULL, bank_rows < 1, first_step < 0, n outside
 * [0, bank_rows], a bank or a destination that is not 16-byte aligned.  HTM_ERR_STATE: a handle without the device's Spatial Pooler. */
int htm_view_sync(htm_handle *view, htm_handle *source);
int htm_bank_rows(htm_handle *h, const uint32_t *device_bank, int32_t bank_rows, int64_t first_step, int32_t n, uint32_t *device_dst);

/* Region stacks: L regions on top of each other, region l + 1 reading region l's active columns.  In
 * reference terms a stack is L HierarchicalTemporalMemory objects with input_dim[l+1] == column_dim[l]; the upper one's step u is
 *   x = np.zeros(column_dim[l], bool); x[sp_state.active_column] = True  for the sp_state (networks.py:29,34) of each of the
 *   lower one's steps u * stride .. (u + 1) * stride - 1;  upper.process(x, learning)          (networks.py:146-149)
 * The link is feed-forward, so the lower region runs a chunk of steps as a recorded run (htm_run_recorded: active_column into a
 * device buffer), htm_pack_columns turns the lists into the upper region's bank, and the upper region runs over it (htm_run),
 * all on one stream and without the host.
 *
 * Bank rows for `dst` (input_dim = the column_dim the lists index) from recorded active-column lists:
 * row (first_row + r) % bank_rows of device_bank, r in [0, n_rows), = OR over j in [0, stride) of the bits
 * device_lists[(r * stride + j) * k + 0..k).  Rows in dst's bank layout (words_per_row of htm_info, pad bits 0).
 * Enqueued on dst's stream; no copy, no wait.
 *
 * A run reads bank row step_index % n_inputs: for a bank that holds exactly the rows of the coming run, pass bank_rows = n_rows
 * and first_row = step_index % bank_rows.  An id outside [0, input_dim) sets no bit and raises bit 64 of htm_info.capacity_error
 * (sticky).  Rows outside the n_rows written keep their contents.  HTM_ERR_ARGUMENT: NULL pointers, k < 1, stride < 1,
 * n_rows < 0, bank_rows < 1, first_row outside [0, bank_rows), a bank that is not 16-byte aligned, an input_dim whose row does
 * not fit the kernel's LDS (above 524 288).  HTM_ERR_STATE: a handle without the device's Spatial Pooler, a column-sharded
 * handle, a handle that is ahead (HTM_RUN_CONTINUE). */
int htm_pack_columns(htm_handle *dst, const int32_t *device_lists, int32_t k, int32_t n_rows, int32_t stride,
                     uint32_t *device_bank, int32_t bank_rows, int32_t first_row);

/* Pooling links (DESIGN.md sections 14 and 29; the definition: bithtm_amd/pooling.py): the link of a region stack that gives the
 * upper region a decaying union of the lower region's columns instead of their OR.  The link's state over a lower region of C
 * columns is persistence uint8[C] and prev (bit c: the column prediction the lower region's last step left), both 0 at first.
 * Per lower step with the active columns A (a row of device_lists) and its column prediction (a row of column_prediction as
 * htm_run_recorded leaves it, ceil(C / 32) words):
 *   P    = max(P - decay, 0)                                                   every column
 *   P[A] = min(ceiling, P[A] + (prev[A] ? predicted_weight : active_weight))
 *   prev = column prediction
 * and per window of `stride` steps
 *   bank row (first_row + r) % bank_rows = a bit for each of the union_bits columns with the largest P among those with P > 0,
 *   ties at the cut to the lower column index (np.lexsort((arange(C), -P))[:union_bits]); fewer positive columns: fewer bits.
 * device_reset_bits (or NULL): bit (first_row + r) % bank_rows set = P and prev are cleared before window r's first step -- the
 * bits the upper region's run takes for the same rows (htm_set_run_resets).
 *
 * htm_pool_columns: n_rows windows, i.e. n_rows * stride rows of device_lists (k ids each) and of device_column_prediction, into
 * n_rows rows of device_bank, with device_bank, bank_rows and first_row exactly as htm_pack_columns takes them; C is dst's
 * input_dim.  device_persistence (C bytes) and device_prev (ceil(C / 32) words) are read at the start and left as the last step
 * leaves them.  device_scratch is the caller's, scratch_bytes of it: a window needs (stride + 8) * 4 * words_per_row bytes, and
 * the call works in batches of as many windows as fit (three launches per batch, the state arrays carrying the state from one
 * batch to the next).  Enqueued on dst's stream; no copy, no wait, no allocation.  An id outside [0, C) counts for nothing and
 * raises bit 64 of htm_info.capacity_error (sticky), as in htm_pack_columns.  Rows outside the n_rows written keep their contents.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued: htm_pack_columns' refusals (NULL pointers -- the reset bits alone may be NULL --, k < 1,
 * stride < 1, n_rows < 0, bank_rows < 1, first_row outside [0, bank_rows), a bank that is not 16-byte aligned); struct_bytes !=
 * sizeof(htm_pool_link); active_weight or predicted_weight outside [0, 255] or both 0; decay or ceiling outside [1, 255];
 * union_bits outside [1, C]; C above HTM_POOL_MAX_COLUMNS; a persistence, prev or scratch address that is not 16-byte aligned; a
 * scratch too small for one window.  HTM_ERR_STATE, nothing enqueued: as htm_pack_columns. */
#define HTM_POOL_MAX_COLUMNS 262144
typedef struct htm_pool_link {
    uint32_t struct_bytes;              /* sizeof(htm_pool_link) */
    int32_t stride;
    int32_t active_weight, predicted_weight;
    int32_t decay, ceiling;
    int32_t union_bits;
    int32_t reserved;                   /* 0 */
} htm_pool_link;
int htm_pool_columns(htm_handle *dst, htm_pool_link link, const int32_t *device_lists, int32_t k, const uint32_t *device_column_prediction,
                     int32_t n_rows, uint8_t *device_persistence, uint32_t *device_prev, const uint32_t *device_reset_bits,
                     void *device_scratch, int64_t scratch_bytes, uint32_t *device_bank, int32_t bank_rows, int32_t first_row);

/* Closed-loop forecasting: what the model expects over the next n steps, its own predicted input fed back
 * as the next input on the device.  With votes = the predicted-input votes of a state (htm_predicted_input above),
 *   encode(votes, min_votes, max_bits):  x = votes >= min_votes; if max_bits > 0 and x.sum() > max_bits, only the max_bits inputs
 *   with the most votes stay set, ties at the cut-off going to the LOWER input index (np.lexsort((arange(I), -votes))[:max_bits]).
 * An input with fewer than min_votes votes is never set: a row may hold fewer than max_bits bits, or none.  Rows are bank rows
 * (words_per_row words, pad bits 0, every word written).
 *
 * htm_encode_votes: row `row` of device_bank (bank_rows rows) = encode(votes of the handle's current state).  After the held-back
 * tail, two launches on the handle's stream; no copy, no wait.  HTM_ERR_STATE as htm_predicted_input; HTM_ERR_ARGUMENT: NULL,
 * min_votes < 1, max_bits < 0, bank_rows < 1, row outside [0, bank_rows), a bank that is not 16-byte aligned.
 *
 * htm_set_run_feedback: the later htm_run / htm_run_recorded / htm_prepare / htm_prepare_recorded calls on exactly this bank and
 * n_inputs, and the htm_group_run calls whose bank for this member is this bank, write behind the step with index s
 *   bank row (s + 1) % n_inputs = encode(votes of the state that step leaves)
 * -- the row step s + 1 reads.  With row s0 % n_inputs seeded by htm_encode_votes, a run of n <= n_inputs - 1 steps from step
 * index s0 is n steps of the loop  x = encode(votes); htm_step(x, learning = 0), and leaves the x of its steps in the bank.  NULL
 * clears the feedback (calls then launch and capture exactly what they did without it).  A feeding call runs unpipelined
 * whatever use_graph says (step s + 1's overlap cannot start before step s's scan; htm_run_plan reports it so) and ignores
 * HTM_RUN_CONTINUE; its graphs are captured once and read the parameters through a descriptor this call fills on the device.
 * While feedback is set, HTM_ERR_ARGUMENT for a run with learning != 0, on another bank or n_inputs, or with reset bits set
 * (htm_set_run_resets); htm_group_step refuses a member with feedback.  A group may mix members with and without feedback.
 * HTM_ERR_STATE on a column-sharded handle, on a handle without the device's own Spatial Pooler and Temporal Memory and while the
 * handle is ahead (HTM_RUN_CONTINUE); HTM_ERR_ARGUMENT for min_votes < 1, max_bits < 0, n_inputs < 1 and a misaligned bank. */
int htm_encode_votes(htm_handle *h, int32_t min_votes, int32_t max_bits, uint32_t *device_bank, int32_t bank_rows, int32_t row);
int htm_set_run_feedback(htm_handle *h, uint32_t *device_bank, int32_t n_inputs, int32_t min_votes, int32_t max_bits);

/* Batched stand-alone Temporal Memory runs: n_steps of
 *   TemporalMemory.process(sp_state, learning=, return_winner_cell=True)   (networks.py:91-128)
 * -- of htm_tm_step with return_winner_cell = 1 -- whose sp_state.active_column are the rows of a bank of lists that is ALREADY
 * IN DEVICE MEMORY: device_lists = int32[n_rows][n], each row n distinct column ids in [0, column_dim), in any order (they are
 * processed in ascending order, as htm_tm_step's); step t reads row t % n_rows, t = the handle's step index, so the rows cycle
 * with the index across calls as htm_run's bank does.  Nothing is copied or synchronised, and what a call leaves -- cell words,
 * winner list, the last scan's State fields, the segment store with its permanences, counters, sticky flags, step index -- is
 * exactly what the n_steps htm_tm_step calls leave.  n (1 <= n <= active_columns) is one value per call; rows of varying
 * length are not available.
 *
 * Per step: the reset launch where reset bits are set, one launch that clears the step's cell words and sorts the step's row
 * into the winner list (htm_tm_feed.h: it reads the step index from the counter block), then the launches of htm_tm_step, then
 * the record launch of a recorded call.  use_graph bit 0: replay hipGraphs of one step or of 16 (one stream, no forked
 * branches; captured once per bank address, n_rows, n, learning flag and the recorded / resetting modes; calls of fewer than
 * BITHTM_EAGER_BELOW steps launch eagerly); the other bits are ignored.  htm_set_run_resets applies as to htm_run: bit r = a
 * reset before every step that reads row r (n_inputs there = n_rows here, HTM_ERR_ARGUMENT otherwise).  As htm_run does, the end
 * of a call copies the segment count into the pinned hint word (no wait).
 *
 * rec: NULL, or as htm_run_recorded's (record i = the i-th step of this call), where records[i].active_columns is n and a row
 * of active_column (active_columns slots, as ever) holds the sorted list in its first n slots and -1 in the rest;
 * column_prediction as there; predicted_columns_before of a reset step is 0.
 *
 * The lists are the caller's contract, checked on the device all the same: a row with a repeated id or an id outside
 * [0, column_dim) never makes a launch read or write out of bounds -- the step runs on the row's valid ids plus the lowest
 * columns not listed -- and raises the sticky bit 128 of htm_info.capacity_error: the results of the call are invalid, and
 * htm_get_info returns HTM_ERR_CAPACITY from then on.
 *
 * HTM_ERR_STATE: a handle without a Temporal Memory, a column-sharded handle, an inference view, a handle that is ahead
 * (HTM_RUN_CONTINUE), one with an open htm_sp_phase or htm_shard_begin step, one with decoding rows or run feedback set
 * (htm_set_run_predicted_input, htm_set_run_feedback), a recorded call at column_dim of 2^24 or more.  HTM_ERR_ARGUMENT: NULL
 * pointers, n_rows < 1, n outside [1, active_columns], n_steps < 0, a wrong rec->struct_bytes or no record buffer, reset bits
 * set for another n_rows, a column_dim whose bitmap does not fit the sorting block's LDS (above 524 032). */
int htm_tm_run(htm_handle *h, const int32_t *device_lists, int32_t n_rows, int32_t n, int32_t n_steps, int32_t learning,
               int32_t use_graph, const htm_run_record *rec);

/* Device-side input noise: the input of example.py:52,
 *   pattern ^ (np.random.rand(input_dim) < p)                                      (example.py:52)
 * a fresh draw per timestep, with np.random.rand replaced by the keyed generator (stream 6, HTM_STREAM_INPUT_NOISE):
 *   flip(seed, step)[i] = i < input_dim and draw24(stream_base(seed, 6, step), i, 0) < threshold24
 * where threshold24 = ceil(p * 2^24), which makes the integer comparison equal to draw24 * 2^-24 < p for every draw.
 *
 * A bulk fill of a ring bank: for step = first_step + r (a uint32: it wraps as the device's step counter does), r in [0, n_rows),
 *   dst_bank row (step % n_dst) = src_bank row (step % n_src) ^ flip(seed, step)
 * in the handle's bank layout (words_per_row of htm_info; pad bits 0 provided the source's are; every word of a written row is
 * written; rows outside the window keep their contents).  A run over (dst_bank, n_dst) from step index first_step then reads,
 * for n_rows steps, the source rows cycled and freshly flipped -- the noise is a function of (seed, step, input) alone, so it
 * never repeats with either bank, and successive windows continue one another.  If the uint32 step wraps inside the window and
 * two of its steps share a ring row, the later step's row stays.
 *
 * Reset bits (htm_set_run_resets), both pointers or neither: src_resets = one bit per source row; ALL ceil(n_dst / 32) words of
 * dst_resets are written -- bit j = the source bit of the step whose row ring row j now holds, 0 for a row outside the window.
 *
 * One launch on the handle's stream behind whatever is already there; no copy, no wait, and no state of the handle is read: it may
 * be called on any handle with the device's own Spatial Pooler (inference views included), also while the handle is ahead
 * (HTM_RUN_CONTINUE) -- the caller then refills the row of the coming step with the words it had.  HTM_ERR_ARGUMENT: NULL banks,
 * src_bank == dst_bank, n_src < 1, n_dst < 1, n_rows outside [0, n_dst], threshold24 above 2^24, exactly one reset pointer, a
 * bank that is not 16-byte aligned.  HTM_ERR_STATE: a handle without the device's Spatial Pooler. */
int htm_bank_noise(htm_handle *h, const uint32_t *src_bank, int32_t n_src, uint32_t *dst_bank, int32_t n_dst,
                   uint32_t first_step, int32_t n_rows, uint32_t seed, uint32_t threshold24,
                   const uint32_t *src_resets, uint32_t *dst_resets);

/* Batched stand-alone Spatial Pooler runs: n_steps of
 *   SpatialPooler.process(input, learning)                                         (networks.py:26-35)
 * -- of htm_sp_step -- whose inputs are the rows of a bank that is ALREADY IN DEVICE MEMORY (htm_bank_upload's layout,
 * words_per_row of htm_info per row): step t reads row t % n_inputs, t = the handle's step index, so the rows cycle with the index
 * across calls as htm_run's bank does.  Nothing is copied or synchronised, and what a call leaves -- permanence rows, connected
 * mask, duty cycle (which moves with learning = 0 too: networks.py:33), step index, and the HTM_F_OVERLAPS / _BOOSTED /
 * _ACTIVE_COLUMN fields of the last step -- is exactly what the n_steps htm_sp_step calls leave.
 *
 * Per step: the launches of htm_sp_step up to the winner list, then one launch with the k winner rows' permanence update
 * (projections.py:23-24) and, in further blocks of the same launch, the step's record: a recorded learning step costs no launch
 * more than an unrecorded one, and a step that neither learns nor records has no such launch (htm_sp_run.h).  use_graph bit 0:
 * replay hipGraphs of one step or of 16 (one stream; captured once per bank address, n_inputs, learning flag and whether
 * recorded -- not per record buffer: the launches read the buffers from a device-side descriptor the call fills first; calls of
 * fewer than BITHTM_EAGER_BELOW steps and calls under htm_profile launch eagerly); the other bits are ignored: a Spatial Pooler
 * alone has nothing to work ahead of -- step t + 1's overlap reads the mask rows step t's learning wrote.
 *
 * rec: NULL (nothing is recorded), or the device buffers of a per-step record, any of them NULL; record i = the i-th step of
 * this call, k = active_columns values per step in the order of the step's winner list (ascending column).  Buffer sizes are the
 * caller's contract, as in htm_run_recorded.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued, the handle as it was: a NULL handle or bank, n_inputs < 1, n_steps < 0, a wrong
 * rec->struct_bytes, a rec with no buffer.  HTM_ERR_STATE, likewise: a handle that also has a Temporal Memory (use htm_run), a
 * handle without a Spatial Pooler, a column-sharded handle, an inference view, a handle that is ahead (HTM_RUN_CONTINUE).
 * n_steps == 0 returns HTM_OK and does nothing.  A call with steps closes an open htm_sp_phase step the way htm_sp_step does: the
 * phases run so far are dropped and the run's first step starts that timestep over. */
typedef struct htm_sp_run_record {
    uint32_t struct_bytes;      /* sizeof(htm_sp_run_record), checked */
    int32_t *active_column;     /* device, [n_steps * active_columns]: sp_state.active_column of each step, ascending; or NULL */
    int32_t *active_overlap;    /* device, [n_steps * active_columns]: overlaps[active_column], same order; or NULL */
    double  *active_boosted;    /* device, [n_steps * active_columns]: boosted_overlaps[active_column], same order; or NULL */
} htm_sp_run_record;

int htm_sp_run(htm_handle *h, const uint32_t *device_inputs, int32_t n_inputs, int32_t n_steps, int32_t learning, int32_t use_graph,
               const htm_sp_run_record *rec);

/* Scalar streams: values in, bank rows out; votes in, a bucket and a score per field out -- so that a
 * stream of numbers stays on the device from the value to the predicted value.  The reference has no encoder: the definition is
 * this project's own, and bithtm_amd/encoders.py is its NumPy form.
 *
 * A field owns the input bits [offset, offset + bits) and sets `width` of them per value:
 *   buckets = bits for a periodic field, else bits - width + 1
 *   scale   = buckets / (maximum - minimum), formed once by the caller in float64 and passed as that double
 *   bucket(v): t = (v - minimum) * scale, two separately rounded IEEE double operations;
 *     non-periodic: a NaN t is missing (-1); else floor(t) clamped to [0, buckets - 1] in double, then converted (+-inf and
 *                   huge values land on the end buckets, v == maximum on the last one)
 *     periodic:     unless -2^31 <= t < 2^31 the value is missing (NaN and +-inf fail the comparison); else (int64)floor(t) mod
 *                   buckets, non-negative
 *   encode:    a bucket b >= 0 sets the bits offset + (b + j) % bits for j < width (a non-periodic field never wraps); a missing
 *              value sets no bit of its field
 *   decode:    score[b] = sum over j < width of votes[offset + (b + j) % bits] for b in [0, buckets); the result is the lowest b
 *              with the largest score, and (-1, 0) where that score is 0.  Votes are counts, never negative; scores are int32.
 *   The value of a bucket is minimum + (b + 0.5) / scale, formed by the caller from the bucket: the device never forms it.
 *
 * htm_bank_encode: bank row first_row + r = encode(device_values row r) for r in [0, n_rows), device_values being
 * double[n_rows][n_fields], row-major, in DEVICE memory, and the bank in the handle's layout (words_per_row of htm_info per row).
 * Every word of a written row is written, pad bits 0; rows outside the window keep their contents.
 * htm_decode_votes: device_out[r][j] = the two int32 (bucket, score) of field j decoded from row r of device_votes, rows of
 * input_dim int32 as htm_set_run_predicted_input writes them; device_out is [n_rows][n_fields][2].
 * Both are one launch on the handle's stream behind whatever is already there; no copy, no wait, and no state of the handle is
 * read: they may be called on any handle with the device's own Spatial Pooler (inference views included), also while the handle
 * is ahead (HTM_RUN_CONTINUE), as htm_bank_noise.  n_rows == 0 returns HTM_OK and does nothing.
 * htm_predicted_value: htm_predicted_input with the votes kept on the device, in a buffer of the handle's: after the held-back
 * tail the votes launch, the decode launch and one synchronising copy of host_out[n_fields][2], (bucket, score) per field.  A
 * state without predictions gives (-1, 0).  HTM_ERR_STATE as htm_predicted_input.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued, the handle as it was: NULL pointers; n_fields outside [1, HTM_SCALAR_MAX_FIELDS]; a field
 * with bits < 1, width outside [1, bits], buckets not as defined or offset < 0; a field that reaches past input_dim; two fields
 * that overlap; a minimum or scale that is not finite, or scale <= 0; n_rows < 0; first_row < 0 or first_row + n_rows >
 * bank_rows; a bank that is not 16-byte aligned (values: 8-byte); for the two decoding calls a field of more than
 * HTM_DECODE_MAX_BITS bits (the prefix sums of a field live in the decode block's LDS).  HTM_ERR_STATE: a handle without the
 * device's Spatial Pooler.
 *
 * Field kinds.  The member `reserved` carries the kind of a field:
 *   reserved == 0     a linear field: all of the above, bit for bit
 *   reserved & 3      the kind otherwise: HTM_FIELD_CATEGORY (1), HTM_FIELD_HASHED (2) or HTM_FIELD_COORDINATE (3, below)
 *   reserved >> 2     the seed of a hashed field or of a coordinate field's head, 0 <= seed < 2^29; it must be 0 anywhere else
 * A category field has `buckets` categories of `width` bits each, buckets * width <= bits (trailing bits stay unused), and is
 * passed with minimum 0 and scale 1:
 *   bucket(v): t = (v - minimum) * scale as above; missing (-1) unless 0 <= floor(t) < buckets -- an unknown id, NaN and +-inf
 *              are missing, NOT clamped
 *   encode:    bucket c sets the bits offset + c * width + j, j < width: no two categories share a bit
 *   decode:    score[c] = sum over j < width of votes[offset + c * width + j]
 * A hashed field (a random distributed scalar field) has any `buckets` >= 1 over its `bits`, 1 <= width <=
 * HTM_HASHED_MAX_WIDTH (width may exceed bits), scale = buckets / (maximum - minimum):
 *   bucket(v): that of a non-periodic linear field
 *   pos(i)   = ((uint64_t)htm_draw32(htm_stream_base(seed, 7, 0), i, 0) * bits) >> 32 for i in [0, buckets + width - 1): the
 *              keyed hash of bithtm_amd/csrc/htm_rng.h, stream 7
 *   encode:    bucket b sets the bits offset + pos(b + j), j < width; positions may collide, so fewer than width bits may be set
 *   decode:    G[i] = votes[offset + pos(i)], score[b] = G[b] + ... + G[b + width - 1] (a collided bit counts once per j)
 * Both decode to the lowest bucket with the largest score, (-1, 0) where that score is 0, as a linear field.
 * HTM_ERR_ARGUMENT, nothing enqueued, besides the cases above (which hold for every kind, `width <= bits` and `buckets` as
 * defined for linear fields only): reserved < 0; an entry of kind 3 outside a coordinate group (below: a lone entry of kind 3
 * is refused as it always was); a seed on a field that is neither hashed nor a coordinate head; periodic != 0 on a field that is
 * not linear; a category field with buckets < 1 or buckets * width > bits; a hashed field with buckets < 1 or width >
 * HTM_HASHED_MAX_WIDTH; for the decoding calls a hashed field with buckets + width - 1 > HTM_DECODE_MAX_BITS (this replaces the
 * cap on `bits` for a hashed field: its prefix sums run over positions, not bits).
 * A caller that left garbage in `reserved` sees a difference to earlier builds of ABI version 4, which ignored the member;
 * a caller that zeroed it, as documented, sees none.
 *
 * Coordinate fields: a 2-D position and a radius in, the `width` highest-ranked cells of the square round
 * the position out -- near positions share most of their bits, positions more than two radii apart next to none.  The field reads
 * THREE value columns (x, y, radius in cells) and is a group of three consecutive table entries, one per column; n_fields, the
 * values' last axis and the decode output's field axis go on counting value columns:
 *   head (x)     minimum = x origin, scale = 1 / resolution, offset, bits >= 1, 1 <= width <= HTM_HASHED_MAX_WIDTH,
 *                buckets = max_radius in [0, HTM_COORD_MAX_RADIUS], periodic 0, reserved = 3 | seed << 2
 *   y            minimum = y origin, scale = 1 / resolution, the head's offset, bits 0, width 0, buckets 0, periodic 0, reserved 3
 *   radius       minimum finite, scale > 0 (0 and 1 for a radius given in cells), the rest as the y entry
 *   cell(v):     t = (v - minimum) * scale; missing unless -2^30 <= t < 2^30 (NaN and +-inf fail); else c = (int32_t)floor(t)
 *   radius(v):   t = (v - minimum) * scale; missing if NaN or t < 0; else r = (int)min(floor(t), (double)max_radius): +inf is max_radius
 *   candidates:  the N = (2r + 1)^2 cells cx - r <= x <= cx + r, cy - r <= y <= cy + r, index i = (y - (cy - r)) * (2r + 1) + (x - (cx - r))
 *   order(x, y) = htm_draw24(htm_stream_base(seed, 8, 0), (uint32_t)x, (uint32_t)y)
 *   bit(x, y)   = ((uint64_t)htm_draw32(htm_stream_base(seed, 8, 1), (uint32_t)x, (uint32_t)y) * bits) >> 32
 *   encode:      the min(width, N) candidates of the largest order, ties at the cut to the lower index i, each set offset +
 *                bit(p); bits may collide; a row in which any of the three values is missing gets no bit of the field
 *   decode:      none: every one of the three columns decodes to (-1, 0)
 * HTM_ERR_ARGUMENT, nothing enqueued: a head (kind 3, bits >= 1) not followed by exactly two continuations (kind 3, bits 0) --
 * the end of the table included; a continuation not behind a head, a third one included; max_radius outside [0,
 * HTM_COORD_MAX_RADIUS]; width outside [1, HTM_HASHED_MAX_WIDTH]; periodic != 0; a continuation with a seed, a width, buckets
 * or an offset other than the head's; and on the head what every kind is held to (inside the row, no overlap, a finite minimum and
 * scale > 0 -- the latter two on the continuations too).  Continuations hold no bits and take no part in the overlap check; no
 * entry of the group is held to HTM_DECODE_MAX_BITS. */
#define HTM_SCALAR_MAX_FIELDS 16
#define HTM_DECODE_MAX_BITS 8192
#define HTM_HASHED_MAX_WIDTH 256
#define HTM_COORD_MAX_RADIUS 127
#define HTM_FIELD_LINEAR 0
#define HTM_FIELD_CATEGORY 1
#define HTM_FIELD_HASHED 2
#define HTM_FIELD_COORDINATE 3
typedef struct htm_scalar_field {
    double minimum, scale;
    int32_t offset, bits, width, buckets, periodic, reserved;
} htm_scalar_field;

int htm_bank_encode(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, const double *device_values, int32_t n_rows,
                    uint32_t *device_bank, int32_t bank_rows, int32_t first_row);
int htm_decode_votes(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, const int32_t *device_votes, int32_t n_rows,
                     int32_t *device_out);
int htm_predicted_value(htm_handle *h, const htm_scalar_field *fields, int32_t n_fields, int32_t *host_out);

/* Live ticks of a model group: one call per tick of n streams whose copies, launches and waits do not
 * depend on n.  Every pointer below is HOST memory; the call returns when the results are there.
 *
 * htm_live_tick: for each member i, in order: a sequence reset (htm_reset) if resets[i] is not 0, then one step on its input
 * row -- row i of values, double[n][n_fields], encoded with the field table as htm_bank_encode encodes it (packed_inputs must be
 * NULL), or row i of packed_inputs as the group's host-fed step takes it (fields NULL, n_fields 0, values NULL).  rows[i] is
 * member i's record of that step, the index of the step and the member's sticky capacity flags after it (what htm_get_info
 * reports as capacity_error).  decoded (optional, only with a field table): int32[n][n_fields][2], (bucket, score) of the
 * votes of the state the step leaves, as htm_predicted_value gives them.  votes (optional): int32[n][input_dim], those votes
 * themselves, as htm_predicted_input gives them.  Decoding rows a member has set (htm_set_run_predicted_input) are neither
 * written nor unset.  learning and use_graph as in the group's batched run (a tick is a call of one step: eager below
 * BITHTM_EAGER_BELOW).  With all members on one stream a tick makes one copy to the device, the launches, one copy back and one
 * wait; the members' segment hints are taken from the result rows.
 * Refused with nothing enqueued and the group usable afterwards: everything the group's batched run refuses of its members
 * (HTM_ERR_STATE: step parities that differ, a member that is ahead or has a step open, reset bits or run feedback set on a
 * member, learning on a group with inference views), and HTM_ERR_ARGUMENT: NULL rows, neither or both of values and
 * packed_inputs, a field table the scalar calls above refuse, decoded without a field table.  A NULL group: HTM_ERR_ARGUMENT.
 *
 * htm_live_reset: htm_reset of every member whose byte in members is not 0 (NULL: all of them), in one launch and without a
 * wait; members of either step parity.  Refused as htm_reset refuses a member (ahead, a step open). */
typedef struct htm_live_row {
    htm_step_record record;
    int64_t step_index;
    int32_t capacity_error;
    int32_t reserved;
} htm_live_row;

int htm_live_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                  const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes);
int htm_live_reset(htm_group *g, const uint8_t *members);

/* Anomaly likelihood on the device (the definition is bithtm_amd/likelihood.py, which the device equals
 * bit for bit): per stream, how improbable the recent short-term average of the raw anomaly score bursting_columns /
 * active_columns is under the distribution of the stream's own recent history.  An htm_likelihood object holds the state of
 * n_streams streams in device memory -- per stream t (scores seen so far, int64), the ring of the last averaging_window raw
 * scores q = (bursting << 16) / active, the ring of the last `history` short-term averages a, the current estimate (mean, std)
 * and whether there is one.  Sequence resets of a model do not touch it.
 *
 * The parameters carry NuPIC's names: learning_period >= 0, estimation_samples >= 1, history in [1, 16384], averaging_window in
 * [1, 64], reestimation_period >= 1.  tail_table513: 513 doubles in HOST memory, TAIL[i] = 0.5 * erfc((i / 64) / sqrt 2), copied
 * at creation (data: the device evaluates no erfc).  The object lives on h's device; every later call takes a handle of that
 * device and enqueues on that handle's stream.
 *
 * The update call: device_records is a HOST array of n_streams DEVICE pointers, each to n_steps htm_step_record (of which
 * active_columns and bursting_columns are read); device_out is DEVICE memory, double[n_streams][n_steps].  The call is enqueued
 * behind h's stream without a wait: ceil(n_steps / 512) launches, each over all streams, and for n_streams > 1 one copy of the
 * pointer table, whatever n_streams is (one stream: its pointer goes by value, no copy).  The table is copied from the caller's
 * array itself, which has been read when the call returns (as htm_group_step reads its rows): the object has no staging of its
 * own and keeps nothing of h -- no stream, no event -- so h may be destroyed as soon as its work is done, and the next call may
 * come through any handle of the device.  n_steps == 0 returns HTM_OK and enqueues nothing.
 * Order across handles is the caller's: calls on one object through handles that share a stream run in the order they were
 * made; before a call through a handle on ANOTHER stream the caller waits for the earlier stream (htm_sync), as for any device
 * buffer two streams use.  The export and import calls wait for the passed handle's stream only.
 * The reset call: the streams whose byte is not 0 (NULL: all) go back to t = 0 with empty rings and no estimate; one launch, no wait.
 * The export and import calls: the whole state to / from HOST memory of exactly htm_likelihood_state_bytes bytes, after a wait for
 * h's stream.  Layout, n = n_streams: int64 t[n]; double mean[n]; double std[n]; int32 flag[n], padded to a multiple of 8 bytes;
 * int32 q_ring[n][averaging_window]; int32 a_ring[n][history], padded to a multiple of 8 bytes.  Ring entry (step mod length)
 * holds that step's value; entries not written since the last reset are 0.
 * The scored tick: htm_live_tick with two further arguments, the object (n_streams = the group's size) and likelihood, HOST
 * double[n]: member i's record of the tick is the next step of stream i.  One launch more than htm_live_tick (klik_tick, grid
 * (1, n), behind the tick's finish launch), n doubles more in the one copy out, no further copy and no further wait;
 * htm_live_tick is this call with both NULL.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued: NULL pointers (a NULL record pointer of a stream included); a wrong struct_bytes; a
 * parameter outside its range; n_streams < 1; n_steps < 0; a handle on another device; a state size that is not
 * htm_likelihood_state_bytes or an imported t < 0; an object whose n_streams differs from the group's size; likelihood
 * without the object or the object without likelihood.  HTM_ERR_STATE: a column-sharded handle. */
typedef struct htm_likelihood htm_likelihood;
typedef struct htm_likelihood_config {
    uint32_t struct_bytes;
    int32_t learning_period, estimation_samples, history, averaging_window, reestimation_period;
} htm_likelihood_config;

int htm_likelihood_create(htm_handle *h, const htm_likelihood_config *cfg, const double *tail_table513, int32_t n_streams, htm_likelihood **out);
void htm_likelihood_destroy(htm_likelihood *lk);
int htm_likelihood_update(htm_likelihood *lk, htm_handle *h, const htm_step_record *const *device_records, int32_t n_steps, double *device_out);
int htm_likelihood_reset(htm_likelihood *lk, htm_handle *h, const uint8_t *streams);
int64_t htm_likelihood_state_bytes(const htm_likelihood *lk);
int htm_likelihood_export(htm_likelihood *lk, htm_handle *h, void *host_state, int64_t bytes);
int htm_likelihood_import(htm_likelihood *lk, htm_handle *h, const void *host_state, int64_t bytes);
int htm_likelihood_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                        const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                        htm_likelihood *lk, double *likelihood);

/* SDR classifier on the device (the definition is bithtm_amd/classifier.py, which the device equals bit for
 * bit): a softmax regression from the cells of the pattern of step t to the bucket seen at step t + h, learned online, one weight
 * table per horizon h, all in integers.  An htm_classifier object holds in device memory the weights W[h][unit][B_pad] (int32 in
 * units of 2^-16, clamped to [-2^30, 2^30], B_pad = buckets rounded up to a multiple of 4: n_steps x units x B_pad x 4 bytes), the
 * ring of the last steps[n_steps - 1] + 1 patterns and the count of patterns since the history was last emptied; the total step count
 * is kept on the host.
 *
 * The config: buckets in [1, 1024]; n_steps in [1, 8] ascending horizons steps[] in [0, 64]; alpha_q = the learning rate in units of
 * 2^-16, in [1, 65536]; units = column_dim * cell_dim of the patterns' model, a multiple of cell_dim; cell_dim in [1, 64]; max_pairs
 * >= 1, the most pairs a step's pattern may have (the ring's row).  exp_table2049: 2049 int32 in HOST memory, T[i] = round(2^30 *
 * exp(-i / 64)), copied at creation (data: the device evaluates no exp).  The object lives on h's device and keeps nothing of h;
 * every later call takes a handle of that device and enqueues on that handle's stream without a wait.  Order across handles on
 * different streams is the caller's, as for htm_likelihood.
 *
 * A pattern is pairs_per_step pairs (int32 index, uint32 word): bit j of word means unit (index / WPC) * cell_dim + (index % WPC)
 * * 32 + j, WPC = ceil(cell_dim / 32) -- the word `index` of a model's cell activation.  A pair with index < 0 or word == 0
 * contributes nothing; the indices of one pattern must be distinct (the caller's promise: a learning step adds to every named row
 * once).  Bits that name no unit of the table are ignored.
 *
 * The update call: device_pairs is DEVICE memory, n_steps x pairs_per_step pairs; device_targets int32[n_targets] in DEVICE memory,
 * step i reading entry (first_step + i) % n_targets (any value outside [0, buckets) is a missing target); device_reset_bits (DEVICE,
 * or NULL: no resets) one bit per entry as htm_set_run_resets takes them: the history is emptied before a step whose bit is set.
 * device_best: DEVICE int32[n_steps][n_horizons][2], per step and horizon the lowest bucket with the largest activation and its
 * probability in units of 2^-16; device_dist: DEVICE int32[n_steps][n_horizons][buckets] or NULL, all probabilities.  learn != 0:
 * two launches per step (kcls_sum, kcls_apply); learn == 0: one launch (kcls_frozen) per 512 steps, the weights unchanged, history
 * and counts advanced as a learning call does.  Successive calls compose: a calls of steps then b are one call of a + b.
 * The reset call empties the history (the weights stay).  read_weights / write_weights: rows [unit0, unit0 + n_units) of one horizon
 * (its index in steps[]) to / from HOST int32[n_units][buckets], after a wait for h's stream.  export / import: everything but the
 * weights to / from HOST memory of exactly htm_classifier_state_bytes bytes, after a wait for h's stream: int64 total; int64 count;
 * then the ring, (int32 index, uint32 word)[ring_len][max_pairs], slot (step mod ring_len) holding that step's pattern, unused pairs
 * (-1, 0).
 *
 * HTM_ERR_ARGUMENT, nothing enqueued: NULL pointers; a wrong struct_bytes; a parameter outside its range; pairs_per_step outside
 * [1, max_pairs]; n_steps < 0; n_targets < 1 or first_step < 0; a handle on another device; a horizon or a range of rows outside the
 * table; a written weight outside [-2^30, 2^30]; a state of another size, or one with count < 0 or count > total.  HTM_ERR_STATE: a
 * column-sharded handle. */
typedef struct htm_classifier htm_classifier;
typedef struct htm_classifier_config {
    uint32_t struct_bytes;
    int32_t buckets, n_steps, alpha_q, units, cell_dim, max_pairs;
    int32_t steps[8];
} htm_classifier_config;

int htm_classifier_create(htm_handle *h, const htm_classifier_config *cfg, const int32_t *exp_table2049, htm_classifier **out);
void htm_classifier_destroy(htm_classifier *clf);
int htm_classifier_update(htm_classifier *clf, htm_handle *h, const void *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                          const int32_t *device_targets, int32_t n_targets, int32_t first_step, const uint32_t *device_reset_bits,
                          int32_t learn, int32_t *device_best, int32_t *device_dist);
int htm_classifier_reset(htm_classifier *clf, htm_handle *h);
int htm_classifier_read_weights(htm_classifier *clf, htm_handle *h, int32_t horizon, int32_t unit0, int32_t n_units, int32_t *host_dst);
int htm_classifier_write_weights(htm_classifier *clf, htm_handle *h, int32_t horizon, int32_t unit0, int32_t n_units, const int32_t *host_src);
int64_t htm_classifier_state_bytes(const htm_classifier *clf);
int htm_classifier_export(htm_classifier *clf, htm_handle *h, void *host_state, int64_t bytes);
int htm_classifier_import(htm_classifier *clf, htm_handle *h, const void *host_state, int64_t bytes);

/* A bank of classifiers: n_streams independent streams of one config in one htm_classifier object -- stream i
 * fed (pairs_i, targets_i, resets_i) equals a one-stream object fed the same, bit for bit -- with every call over all streams in the
 * launches of one.  Device memory, member-major: weights [n_streams][n_steps][units][B_pad], rings [n_streams][ring_len][max_pairs],
 * counts [n_streams], and the learning accumulators per stream and horizon; one total on the host, since every call advances all
 * streams by the same number of steps.  n_streams is in [1, 65535 / n_steps] (the member shares grid y with the horizon).
 *
 * share_weights_of (or NULL): an existing one-stream htm_classifier of the same config on h's device.  The new object then reads
 * that object's weight table where it lies -- nothing is copied, and what the other object learns later is seen here -- and owns only
 * rings, counts and accumulators.  The table is reference-counted inside the library: either object may be destroyed first
 * (htm_classifier_destroy destroys a bank too).  The order between the other object's learning calls and this object's calls on
 * different streams is the caller's.
 *
 * The update call: device_pairs, device_targets and device_reset_bits (or NULL: no resets) are HOST arrays of n_streams DEVICE
 * pointers, each what the one-stream update call takes; they are copied as one pointer table per call, read before the call returns
 * (n_streams == 1: passed by value, no copy).  device_best: DEVICE int32[n_streams][n_steps][n_horizons][2]; device_dist: DEVICE
 * int32[n_streams][n_steps][n_horizons][buckets] or NULL.  Enqueued on h's stream without a wait.  learn != 0: two launches per step
 * (kgcls_sum, kgcls_apply, grid y = n_streams x n_horizons); learn == 0: one launch (kgcls_frozen) per min(512, 65535 / (n_streams x
 * n_horizons)) steps.  The reset call empties the history of the streams whose byte of streams (HOST uint8[n_streams]) is not 0, or of
 * all (NULL).  read_weights / write_weights take the stream besides what the one-stream calls take.  export / import: HOST memory of
 * exactly htm_classifiers_state_bytes bytes: int64 total; int64 count[n_streams]; then the rings.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued: what the one-stream calls refuse; n_streams outside its range; a share_weights_of of another
 * config, with more than one stream or on another device; a NULL entry of a pointer array; a stream outside [0, n_streams); the
 * one-stream update, reset, weights, export or import call on an object with more than one stream.  HTM_ERR_STATE: learn != 0 on an
 * object that shares its weights, whatever its n_streams and through either update call (the owner alone writes its table); weights
 * written through an object that shares them. */
int htm_classifiers_create(htm_handle *h, const htm_classifier_config *cfg, const int32_t *exp_table2049, int32_t n_streams,
                           htm_classifier *share_weights_of, htm_classifier **out);
int htm_classifiers_update(htm_classifier *clf, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                           const int32_t *const *device_targets, int32_t n_targets, int32_t first_step, const uint32_t *const *device_reset_bits,
                           int32_t learn, int32_t *device_best, int32_t *device_dist);
int htm_classifiers_reset(htm_classifier *clf, htm_handle *h, const uint8_t *streams);
int htm_classifiers_read_weights(htm_classifier *clf, htm_handle *h, int32_t stream, int32_t horizon, int32_t unit0, int32_t n_units, int32_t *host_dst);
int htm_classifiers_write_weights(htm_classifier *clf, htm_handle *h, int32_t stream, int32_t horizon, int32_t unit0, int32_t n_units,
                                  const int32_t *host_src);
int64_t htm_classifiers_state_bytes(const htm_classifier *clf);
int htm_classifiers_export(htm_classifier *clf, htm_handle *h, void *host_state, int64_t bytes);
int htm_classifiers_import(htm_classifier *clf, htm_handle *h, const void *host_state, int64_t bytes);

/* Pattern capture for the classifier: after htm_set_run_active_cells(h, device_pairs), an htm_run_recorded call of n steps writes
 * n x k x WPC pairs (int32 index, uint32 word) into device_pairs (DEVICE memory): row i holds step i's active-cell words of its k
 * active columns in active_column order -- index = column * WPC + w, word = word `index` of the step's cell activation, k =
 * active_columns, WPC = ceil(cell_dim / 32) -- which is what htm_classifier_update takes with pairs_per_step = k * WPC.  One small
 * launch (kcls_capture) directly behind each step's record launch; graphs are captured once and read the rows through a device
 * descriptor, which this call fills with one 8-byte copy on h's stream.  NULL clears the rows: calls then launch and capture exactly
 * what they did before.  While rows are set: htm_run (and htm_prepare) without a record is HTM_ERR_ARGUMENT; htm_tm_run and a group
 * call with such a member are HTM_ERR_STATE.  Setting rows on a column-sharded handle, or on one without the device's own Spatial
 * Pooler and Temporal Memory, is HTM_ERR_STATE. */
int htm_set_run_active_cells(htm_handle *h, void *device_pairs);

/* Pattern capture for a group: device_pairs is a HOST array of one DEVICE pointer per member (read before the
 * call returns; one copy on the group's stream fills the group's table of capture descriptors).  After it a recorded htm_group_run (or
 * htm_group_step) of n steps leaves each member's n x k x WPC pairs in its rows, exactly as htm_set_run_active_cells does for a
 * recorded htm_run of the member alone: one launch (kgcls_capture, grid y = member) directly behind each step's record launch,
 * inside the group's graphs, which are captured once per mode.  NULL clears the rows: calls then launch what they did before.  While
 * rows are set, a group run or step without records is HTM_ERR_ARGUMENT.  HTM_ERR_ARGUMENT: a NULL entry.  HTM_ERR_STATE: a
 * column-sharded member, or one without the device's own Spatial Pooler and Temporal Memory.  A member with rows of its own
 * (htm_set_run_active_cells) still makes every group call HTM_ERR_STATE. */
int htm_set_group_run_active_cells(htm_group *g, void *const *device_pairs);

/* Stacks of model groups: the links of B streams' hierarchies, every launch covering all members (grid y =
 * member).  dst is the group of the UPPER level's members.  For member i the effect is exactly that of htm_pack_columns /
 * htm_pool_columns on member i with the i-th entries of the arrays: its bank rows, the rows left untouched, the persistence and prev
 * it ends with, and bit 64 of ITS htm_info.capacity_error for an id outside its range -- no other member's.
 * device_lists, device_banks, device_column_prediction, device_persistence, device_prev, device_reset_bits (the array, or any of its
 * entries, may be NULL: no reset bits) and first_rows are HOST arrays of one entry per member, read before the call returns: they go
 * to the device as ONE table per call (one copy on the group's stream into a buffer the group keeps; the batches' offsets go by
 * value).  k, n_rows, stride / link, bank_rows are the same for every member.  Enqueued on the group's stream: no wait, and no
 * allocation once the group's table has its size.
 * htm_group_pack_columns: ONE launch (kgrp_pack_columns, grid (n_rows, B)).
 * htm_group_pool_columns: per batch three launches whatever B is (kgrp_pack_columns at stride 1, kgpool_scan, kgpool_select); a
 * batch is floor(scratch_bytes / (B * (stride + 8) * 4 * words_per_row)) windows of every member.  The scratch: member i's part
 * begins i * batch * (stride + 8) * 4 * words_per_row bytes in and is laid out as htm_pool_columns lays out a batch (batch * stride
 * bitmap rows, then batch snapshot rows of 32 * words_per_row bytes).
 * HTM_ERR_ARGUMENT, nothing enqueued: everything the solo entries refuse, the alignment checked per member; a NULL array or a
 * NULL entry (but the reset bits); a first_rows[i] outside [0, bank_rows); a scratch too small for one window of all members; more
 * than 65535 members.  HTM_ERR_STATE, nothing enqueued: a member without the device's own Spatial Pooler, a column-sharded member, a
 * member that is ahead (HTM_RUN_CONTINUE), a member that enqueues on another stream than the group's. */
int htm_group_pack_columns(htm_group *dst, const int32_t *const *device_lists /* HOST array (as every array here): one DEVICE pointer per member */,
                           int32_t k, int32_t n_rows, int32_t stride,
                           uint32_t *const *device_banks, int32_t bank_rows, const int32_t *first_rows);
int htm_group_pool_columns(htm_group *dst, htm_pool_link link, const int32_t *const *device_lists, int32_t k,
                           const uint32_t *const *device_column_prediction, int32_t n_rows,
                           uint8_t *const *device_persistence, uint32_t *const *device_prev,
                           const uint32_t *const *device_reset_bits /* or NULL (entries may be NULL too) */,
                           void *device_scratch, int64_t scratch_bytes,
                           uint32_t *const *device_banks, int32_t bank_rows, const int32_t *first_rows);

/* The classified tick: htm_likelihood_tick -- which is this call with the five classifier arguments NULL / 0 --
 * with a bank of classifiers riding on it; lk and likelihood may be NULL (an unscored, classified tick).  clf: a bank of as many
 * streams as the group has members, on the group's device, made for the members' column_dim x cell_dim with max_pairs >= k x WPC.
 * targets: HOST int32[B], member i's bucket of this tick (outside [0, buckets): missing); it rides in the tick's pinned staging block:
 * still ONE copy in.  best: HOST int32[B][n_horizons][2]; dist: HOST int32[B][n_horizons][buckets] or NULL; they ride in the tick's
 * result block: still ONE copy out and ONE wait.  Launches: kgcls_capture behind the step's record launch (inside the tick's graph,
 * which is keyed on it), then, behind the finish launch (and the likelihood launch of a scored tick), kgcls_sum + kgcls_apply when
 * learn != 0, or kgcls_frozen over one step otherwise: 3 launches more for a learning tick, 2 for a frozen one, at every B.  A
 * member's reset flag also empties its stream's history before its pattern enters it; the object's total advances by one.
 * Refused with nothing enqueued, the group staying usable -- HTM_ERR_ARGUMENT: clf, targets and best not given together, dist without
 * them; n_streams other than the group's size; another device; another column_dim or cell_dim than the members'; max_pairs below k x
 * WPC.  HTM_ERR_STATE: learn != 0 on an object that shares its weights; a member that is column-sharded or lacks the device's own
 * Spatial Pooler and Temporal Memory. */
int htm_classifiers_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                         const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                         htm_likelihood *lk, double *likelihood, htm_classifier *clf, const int32_t *targets, int32_t learn, int32_t *best,
                         int32_t *dist);

/* KNN classifier over active-cell patterns (the definition is bithtm_amd/knn.py, which the device equals bit
 * for bit): the patterns of labelled steps are stored, a later step gets the label most of its k nearest stored patterns carry.  An
 * htm_knn object holds in device memory the store -- `capacity` slots of max_pairs (int32 index, uint32 word) pairs (unused pairs
 * (-1, 0)), an int32 label and an int64 stamp (the object's step total at the storing step) per slot -- and the scratch of an update;
 * the slots in use (`count`) and the step total are kept on the HOST: every store is decided by what the host knows, nothing is read
 * back.  Patterns are htm_classifier_update's (htm_set_run_active_cells captures them); overlap(P, Q) is the sum of popcount(wP & wQ)
 * over the indices both hold, live bits only.
 *
 * htm_knn_update: n_steps steps over device_pairs [n_steps][pairs_per_step] (DEVICE memory), step i with the label device_labels
 * [(first_step + i) % n_labels] (outside [0, labels): none).  Each step first infers over the store as it is -- candidates: the slots
 * with overlap >= min_overlap; neighbours: the first k by (overlap descending, slot ascending) -- into device_best [n_steps][5] (the
 * lowest label with the most votes, its votes, the first neighbour's overlap, slot and the low 32 bits of its stamp; -1, 0, 0, -1, -1
 * without a neighbour) and device_votes [n_steps][labels] (or NULL); then, with learn != 0 and a label, its pattern goes into slot
 * `count` (the store never overwrites).  Everything is enqueued on h's stream, nothing waits: two launches per call that stores
 * (kknn_place, kknn_append), then per chunk of 64 steps kknn_distance_lds and kknn_select -- or, where one dense table of column_dim x
 * WPC words exceeds 48 KiB, kknn_scatter, kknn_distance_global, kknn_select, kknn_scatter.  A learning call takes its labels from
 * htm_knn_labels: that call copies n_labels HOST labels into the object's own device array (on h's stream; the words are read before
 * it returns), keeps them on the host and returns the device array's address in *device_labels; a call with learn != 0 must pass
 * that address and that n_labels, so that the host can count what the call stores.  A call with learn == 0 may read any device array.
 * htm_knn_reset empties the store (count = 0; the total stays).  htm_knn_export / _import copy the state to / from HOST memory after a
 * wait for h's stream: int64 total; int64 count; then count x max_pairs pairs, count int64 stamps, count int32 labels -- 16 + count x
 * (8 max_pairs + 12) bytes, htm_knn_info's state_bytes.  An object may be used through any handle of its device; the order between
 * calls is that of the streams they come on.
 *
 * HTM_ERR_ARGUMENT, nothing enqueued, the object as it was: NULL pointers; a wrong struct_bytes; labels outside [1, 1024], k outside
 * [1, 64], min_overlap outside [1, 65535], capacity outside [1, 2^20], cell_dim outside [1, 64], units no positive multiple of
 * cell_dim, max_pairs outside [1, 2047]; pairs_per_step outside [1, max_pairs]; n_steps < 0, n_labels < 1, first_step < 0; a learning
 * call with other labels than htm_knn_labels'; a handle on another device; a state of another size than its own count says, with count
 * above capacity, a label outside [0, labels), or stamps that do not ascend below total.  HTM_ERR_CAPACITY, likewise: a call whose
 * labelled steps would take count past capacity.  HTM_ERR_STATE: a column-sharded handle. */
typedef struct htm_knn htm_knn;
typedef struct htm_knn_config {
    uint32_t struct_bytes;
    int32_t labels, k, min_overlap, capacity, units, cell_dim, max_pairs;
} htm_knn_config;
typedef struct htm_knn_info_t {
    uint32_t struct_bytes;
    int32_t labels, k, min_overlap, capacity, units, cell_dim, max_pairs;
    int32_t count;                  /* slots in use */
    int32_t table_in_lds;           /* 1: kknn_distance_lds; 0: the global-table form */
    int32_t queries_per_block;      /* queries one block of the distance launch stages: the store is read once per that many steps */
    int32_t bin_shift;              /* the select's histogram bins overlaps >> bin_shift */
    int64_t total;                  /* steps seen */
    int64_t state_bytes;            /* of htm_knn_export now */
    int64_t device_bytes;           /* device memory the object holds */
} htm_knn_info_t;

int htm_knn_create(htm_handle *h, const htm_knn_config *cfg, htm_knn **out);
void htm_knn_destroy(htm_knn *knn);
int htm_knn_labels(htm_knn *knn, htm_handle *h, const int32_t *host_labels, int32_t n_labels, const int32_t **device_labels);
int htm_knn_update(htm_knn *knn, htm_handle *h, const void *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                   const int32_t *device_labels, int32_t n_labels, int32_t first_step, int32_t learn, int32_t *device_best,
                   int32_t *device_votes);
int htm_knn_reset(htm_knn *knn, htm_handle *h);
int htm_knn_export(htm_knn *knn, htm_handle *h, void *host_state, int64_t bytes);
int htm_knn_import(htm_knn *knn, htm_handle *h, const void *host_state, int64_t bytes);
int htm_knn_info(const htm_knn *knn, htm_knn_info_t *out);

/* Banks of KNN classifiers (the definition is bithtm_amd/knn.py's KNNBankDefinition): n_streams independent
 * stores of one config in one htm_knn object, member-major in device memory, stepped by one launch sequence whatever n_streams is;
 * stream i equals a one-stream object fed the same.  The streams' counts and the one step total are the HOST's.  The object is
 * destroyed with htm_knn_destroy.
 *
 * htm_knns_create: share_store_of == NULL: n_streams own stores.  The scratch of an update -- the overlaps [n][chunk][capacity] of 16
 * bits and, where a table exceeds 48 KiB, the tables [n][chunk][words] -- is bounded: chunk, the query steps per launch, is the
 * largest power of two <= 64 whose scratch fits 256 MiB with n x chunk <= 65 535.  share_store_of: a one-stream object of the same
 * config and device -- the n_streams streams are frozen (learn != 0: HTM_ERR_STATE) and infer over THAT object's store as it is at
 * each call, every slot in [0, count) seen; nothing is copied, the store lives until the last object that reads it is destroyed, and
 * the bank owns only its scratch (under the same budget: refused where one query's does not fit).  Its streams' queries are one flat batch: a block of the distance launch streams the store once
 * per queries_per_block queries, whichever stream they belong to; device_pairs[i] must lie one behind the other in stream order.
 *
 * htm_knns_labels: host labels [n][n_labels] into the object's own device array, as htm_knn_labels.  htm_knns_update: device_pairs
 * holds n_streams DEVICE addresses (a host array), each [n_steps][pairs_per_step]; stream i's step j reads label
 * device_labels[i][(first_step + j) % n_labels] (device_labels may be NULL with learn == 0); device_best is [n][n_steps][5],
 * device_votes [n][n_steps][labels] or NULL.  One copy (the table of addresses and per-stream counts), then kgknn_place and
 * kgknn_append when any stream stores, and per chunk kgknn_distance_lds, kgknn_select (or kgknn_scatter, kgknn_distance_global,
 * kgknn_select, kgknn_scatter).  htm_knns_reset empties the stores `streams` names (uint8 [n]; NULL: all); the total stays.
 * htm_knns_export / _import: int64 total; int64 count[n]; the streams' pairs, then their int64 stamps, then their int32 labels, each
 * in stream order -- htm_knns_info's state_bytes (a sharing bank: counts 0).  htm_knns_info also copies the n counts to `counts`
 * (or NULL).
 *
 * Refused with nothing enqueued and every store as it was: what the one-stream calls refuse; n_streams outside [1, 65535]; a scratch
 * that does not fit at chunk 1; share_store_of of another config, a bank, or another device; HTM_ERR_CAPACITY when ANY stream's
 * labelled steps would take it past capacity; HTM_ERR_STATE for the htm_knn_ labels, update, reset, export and import calls on a
 * bank and the htm_knns_ calls on a one-stream object. */
typedef struct htm_knns_info_t {
    uint32_t struct_bytes;
    int32_t labels, k, min_overlap, capacity, units, cell_dim, max_pairs;
    int32_t n_streams;
    int32_t shared;           /* 1: the streams read another object's store */
    int32_t chunk;                  /* query steps per launch */
    int32_t table_in_lds, queries_per_block, bin_shift;
    int32_t max_count;              /* the largest count (a sharing bank: the source's count) */
    int32_t reserved;
    int64_t total;
    int64_t state_bytes;            /* of htm_knns_export now */
    int64_t device_bytes;           /* device memory the object holds */
    int64_t scratch_bytes;          /* ... of which the scratch of an update */
} htm_knns_info_t;

int htm_knns_create(htm_handle *h, const htm_knn_config *cfg, int32_t n_streams, htm_knn *share_store_of, htm_knn **out);
int htm_knns_labels(htm_knn *knn, htm_handle *h, const int32_t *host_labels, int32_t n_labels, const int32_t **device_labels);
int htm_knns_update(htm_knn *knn, htm_handle *h, const void *const *device_pairs, int32_t pairs_per_step, int32_t n_steps,
                    const int32_t *device_labels, int32_t n_labels, int32_t first_step, int32_t learn, int32_t *device_best,
                    int32_t *device_votes);
int htm_knns_reset(htm_knn *knn, htm_handle *h, const uint8_t *streams);
int htm_knns_export(htm_knn *knn, htm_handle *h, void *host_state, int64_t bytes);
int htm_knns_import(htm_knn *knn, htm_handle *h, const void *host_state, int64_t bytes);
int htm_knns_info(const htm_knn *knn, htm_knns_info_t *out, int32_t *counts);

/* htm_classifiers_tick with a bank of KNN classifiers riding on it: the tick's captured patterns are the streams' next step.  lk,
 * likelihood and clf, targets, best, dist may be NULL (each group as in htm_classifiers_tick); with clf and knn the step's patterns
 * are captured once.  labels: HOST int32 [n], each member's label of this tick (outside [0, labels): none; NULL with knn_learn == 0);
 * knn_best: HOST int32 [n][5]; knn_votes: HOST int32 [n][labels] or NULL.  The host knows every label, so it knows every stream's
 * slot: the labels, the counts and the slots ride in the tick's staging copy and there is no place launch -- still one copy in, one
 * copy out and one wait, and behind the tick's launches kgknn_append (when any stream stores), kgknn_distance_lds and kgknn_select
 * (two kgknn_scatter more in the global-table form), whatever n is; a sharing bank: kknn_distance_lds and kknn_select over the n
 * queries as one batch.  A member's reset flag does not touch its store.  Refused with nothing enqueued: what htm_classifiers_tick
 * refuses; a one-stream object; another stream count, device or shape than the group's; knn_learn != 0 on a sharing bank
 * (HTM_ERR_STATE) or without labels; a labelled tick of a stream at capacity (HTM_ERR_CAPACITY). */
int htm_knns_tick(htm_group *g, const double *values, const htm_scalar_field *fields, int32_t n_fields, const uint32_t *packed_inputs,
                  const uint8_t *resets, int32_t learning, int32_t use_graph, htm_live_row *rows, int32_t *decoded, int32_t *votes,
                  htm_likelihood *lk, double *likelihood, htm_classifier *clf, const int32_t *targets, int32_t learn, int32_t *best,
                  int32_t *dist, htm_knn *knn, const int32_t *labels, int32_t knn_learn, int32_t *knn_best, int32_t *knn_votes);

#ifdef __cplusplus
}
#endif
#endif /* BITHTM_HIP_H */
