"""ctypes binding of libbithtm_hip.so (include/bithtm_hip.h).  No fallback: if the HIP
library is missing or cannot be loaded the import fails loudly."""

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbithtm_hip.so")
ABI_VERSION = 4


class HtmConfig(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_uint32), ("device", C.c_int32),
        ("input_dim", C.c_int32), ("column_dim", C.c_int32), ("cell_dim", C.c_int32),
        ("active_columns", C.c_int32), ("enable_sp", C.c_int32), ("enable_tm", C.c_int32),
        ("sp_permanence_threshold", C.c_double), ("sp_delta_on", C.c_double), ("sp_delta_off", C.c_double),
        ("boost_coefficient", C.c_float), ("duty_momentum", C.c_float), ("duty_increment", C.c_float),
        ("tm_learn_active", C.c_double), ("tm_learn_inactive", C.c_double),
        ("tm_punish_active", C.c_double), ("tm_punish_inactive", C.c_double),
        ("tm_learn_prune", C.c_int32), ("tm_punish_prune", C.c_int32),
        ("tm_permanence_initial", C.c_float), ("tm_permanence_threshold", C.c_float),
        ("segment_activation_threshold", C.c_int32), ("segment_matching_threshold", C.c_int32),
        ("segment_sampling_synapses", C.c_int32),
        ("segment_capacity", C.c_int32), ("segment_capacity_local", C.c_int32), ("segment_slots", C.c_int32),
        ("seed", C.c_uint32), ("shard_rank", C.c_int32), ("shard_world", C.c_int32), ("use_caller_stream", C.c_int32),
        ("stream", C.c_void_p),
    ]


class HtmInfo(C.Structure):
    _fields_ = [
        ("step_index", C.c_int64), ("segments", C.c_int32), ("local_segments", C.c_int32), ("matching_segments", C.c_int32),
        ("winner_cells", C.c_int32), ("active_cells", C.c_int32), ("has_distal_state", C.c_int32),
        ("has_winner_cells", C.c_int32), ("capacity_error", C.c_int32), ("words_per_row", C.c_int32),
        ("new_segment_requests", C.c_int32), ("recycled_segments", C.c_int32), ("appended_segments", C.c_int32),
        ("work_items", C.c_int32), ("select_fallbacks", C.c_int32), ("candidate_exact_steps", C.c_int32), ("hot_select_steps", C.c_int32),
        ("select_zoom_steps", C.c_int32),
    ]


class HtmStepRecord(C.Structure):
    _fields_ = [(name, C.c_int32) for name in (
        "active_columns", "bursting_columns", "predicted_columns_before", "predicted_columns", "active_cells", "winner_cells",
        "segments", "new_segments")]


class HtmRunRecord(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("records", C.c_void_p), ("active_column", C.c_void_p), ("column_prediction", C.c_void_p)]


class HtmSpRunRecord(C.Structure):
    _fields_ = [("struct_bytes", C.c_uint32), ("active_column", C.c_void_p), ("active_overlap", C.c_void_p), ("active_boosted", C.c_void_p)]


class HtmScalarField(C.Structure):
    _fields_ = [("minimum", C.c_double), ("scale", C.c_double)] + [(name, C.c_int32) for name in (
        "offset", "bits", "width", "buckets", "periodic", "reserved")]


class HtmLiveRow(C.Structure):
    """htm_live_row: a member's row of a live tick (htm_live_tick) -- the htm_step_record counters, the step's index, the flags."""
    _fields_ = HtmStepRecord._fields_ + [("step_index", C.c_int64), ("capacity_error", C.c_int32), ("reserved", C.c_int32)]


class HtmLikelihoodConfig(C.Structure):
    """htm_likelihood_config: the five parameters of the anomaly likelihood (likelihood.PARAMETERS order)."""
    _fields_ = [("struct_bytes", C.c_uint32)] + [(name, C.c_int32) for name in (
        "learning_period", "estimation_samples", "history", "averaging_window", "reestimation_period")]


class HtmClassifierConfig(C.Structure):
    """htm_classifier_config: the SDR classifier's parameters (buckets, the horizons, the learning rate in units of 2^-16, the
    patterns' geometry and the most pairs a pattern may have)."""
    _fields_ = [("struct_bytes", C.c_uint32)] + [(name, C.c_int32) for name in (
        "buckets", "n_steps", "alpha_q", "units", "cell_dim", "max_pairs")] + [("steps", C.c_int32 * 8)]


class HtmKnnConfig(C.Structure):
    """htm_knn_config: the KNN classifier's parameters (labels, k, the least overlap of a candidate, the slots of the store, the
    patterns' geometry and the most pairs a pattern may have)."""
    _fields_ = [("struct_bytes", C.c_uint32)] + [(name, C.c_int32) for name in (
        "labels", "k", "min_overlap", "capacity", "units", "cell_dim", "max_pairs")]


class HtmKnnInfo(C.Structure):
    """htm_knn_info_t: the parameters again, the slots in use, the form of the distance launch, the step total and the sizes."""
    _fields_ = HtmKnnConfig._fields_ + [(name, C.c_int32) for name in ("count", "table_in_lds", "queries_per_block", "bin_shift")] + [
        (name, C.c_int64) for name in ("total", "state_bytes", "device_bytes")]


class HtmKnnsInfo(C.Structure):
    """htm_knns_info_t: a bank's parameters, its streams, whether they share a store, the chunk, the form of the distance launch,
    the largest count, the step total and the sizes."""
    _fields_ = HtmKnnConfig._fields_ + [(name, C.c_int32) for name in (
        "n_streams", "shared", "chunk", "table_in_lds", "queries_per_block", "bin_shift", "max_count", "reserved")] + [
        (name, C.c_int64) for name in ("total", "state_bytes", "device_bytes", "scratch_bytes")]


class HtmPoolLink(C.Structure):
    """htm_pool_link: the parameters of a pooling link (pooling.PoolingLink.PARAMETERS order)."""
    _fields_ = [("struct_bytes", C.c_uint32)] + [(name, C.c_int32) for name in (
        "stride", "active_weight", "predicted_weight", "decay", "ceiling", "union_bits", "reserved")]


POOL_MAX_COLUMNS = 256 * 1024               # HTM_POOL_MAX_COLUMNS (csrc/htm_pool.h): the most lower columns htm_pool_columns serves
POOL_SCRATCH_BYTES = 256 << 20              # the most scratch a stack gives a pooled link's htm_pool_columns calls
KNNS_SCRATCH_BYTES = 256 << 20              # HTM_KNNS_SCRATCH_BYTES (csrc/htm_knn_bank.h): the most scratch a bank's update may hold
KNNS_MAX_STREAMS = 65535                    # HTM_KNNS_MAX_STREAMS
KNN_CHUNK = 64                              # HTM_KNN_CHUNK (csrc/htm_knn.h): query steps per launch of htm_knn_update
KNN_SLOTS = 256                             # HTM_KNN_SLOTS: slots per block of the distance launch
KNN_QUERIES = 8                             # HTM_KNN_QUERIES: queries a block stages at most
KNN_TABLE_BYTES = 48 * 1024                 # HTM_KNN_TABLE_BYTES: LDS for a block's staged tables
KNN_BINS = 2048                             # HTM_KNN_BINS: bins of the select's histogram
CLASSIFIER_CHUNK = 512                      # HTM_CLASSIFIER_CHUNK (csrc/htm_classifier.h): steps per launch of a frozen htm_classifier_update
CLASSIFIER_PAIRS = 16                       # HTM_CLASSIFIER_PAIRS: pairs of a pattern per block
LIKELIHOOD_CHUNK = 512                      # HTM_LIKELIHOOD_CHUNK (csrc/htm_likelihood.h): steps per launch of htm_likelihood_update

# htm_field
F_ACTIVE_COLUMN, F_OVERLAPS, F_BOOSTED, F_DUTY_CYCLE, F_CELL_ACTIVATION, F_CELL_PREDICTION = 1, 2, 3, 4, 5, 6
F_WINNER_WORDS, F_BURSTING, F_WINNER_CELL, F_SEG_CELL, F_SEG_NSYN, F_SEG_PRESYN, F_SEG_PERM = 7, 8, 9, 10, 11, 12, 13
F_SEGCOUNT, F_SEG_POTENTIAL, F_MATCH_SEGMENT, F_MATCH_INFO, F_MATCH_JITTER, F_CELL_MAX_JITTER = 14, 15, 16, 17, 18, 19
F_SEG_GID = 20
F_RECYCLABLE_COUNTS = 21                    # read only
PLAN_GRAPH, PLAN_PIPELINED, PLAN_LEAN, PLAN_SCAN_LARGE = 1, 2, 4, 8
SP_OVERLAP, SP_BOOST, SP_SELECT, SP_ACTIVE, SP_LEARN, SP_DUTY, SP_COMMIT = 1, 2, 3, 4, 5, 6, 7

EXPORTS = {
    "htm_abi_version": (C.c_int, []),
    "htm_create": (C.c_int, [C.POINTER(HtmConfig), C.POINTER(C.c_void_p)]),
    "htm_destroy": (None, [C.c_void_p]),
    "htm_last_error": (C.c_char_p, [C.c_void_p]),
    "htm_sp_set_permanence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_set_epsilon": (C.c_int, [C.c_void_p, C.c_float]),
    "htm_sp_get_permanence": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "htm_sp_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "htm_sp_phase": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "htm_tm_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "htm_tm_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "htm_tm_scan": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_tm_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HtmRunRecord)]),
    "htm_sp_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HtmSpRunRecord)]),
    "htm_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_run_recorded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HtmRunRecord)]),
    "htm_prepare_recorded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_reset": (C.c_int, [C.c_void_p]),
    "htm_set_run_resets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "htm_predicted_input": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_set_run_predicted_input": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_graph_count": (C.c_int, [C.c_void_p]),
    "htm_run_plan": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "htm_bank_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "htm_shard_record_bytes": (C.c_int64, [C.c_void_p]),
    "htm_shard_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "htm_shard_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "htm_shard_unique_id": (C.c_int, [C.c_void_p]),
    "htm_shard_comm_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_shard_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "htm_shard_comm_size": (C.c_int, [C.c_void_p]),
    "htm_shard_graph_ok": (C.c_int, [C.c_void_p]),
    "htm_shard_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_shard_group_run": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_rccl_selftest": (C.c_int, [C.c_int32]),
    "htm_keyed_draws": (C.c_int, [C.c_uint32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "htm_shard_group_step": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int32]),
    "htm_populate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_uint32]),
    "htm_sync": (C.c_int, [C.c_void_p]),
    "htm_sp_planes_check": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "htm_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "htm_get_info": (C.c_int, [C.c_void_p, C.POINTER(HtmInfo)]),
    "htm_read": (C.c_int64, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "htm_read_rows": (C.c_int64, [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]),
    "htm_import_begin": (C.c_int, [C.c_void_p, C.c_int64]),
    "htm_write": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "htm_import_commit": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "htm_profile": (C.c_int, [C.c_void_p, C.c_int32]),
    "htm_profile_read": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64)]),
    "htm_trace_read": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_group_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_void_p)]),
    "htm_group_destroy": (None, [C.c_void_p]),
    "htm_group_last_error": (C.c_char_p, [C.c_void_p]),
    "htm_group_run": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(HtmRunRecord)]),
    "htm_group_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(HtmRunRecord)]),
    "htm_create_view": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "htm_device_bytes": (C.c_int64, [C.c_void_p]),
    "htm_view_sync": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_bank_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    "htm_pack_columns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_pool_columns": (C.c_int, [C.c_void_p, HtmPoolLink, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_encode_votes": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_set_run_feedback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "htm_bank_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_void_p]),
    "htm_bank_encode": (C.c_int, [C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]),
    "htm_decode_votes": (C.c_int, [C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "htm_predicted_value": (C.c_int, [C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p]),
    "htm_live_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "htm_live_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_likelihood_create": (C.c_int, [C.c_void_p, C.POINTER(HtmLikelihoodConfig), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "htm_likelihood_destroy": (None, [C.c_void_p]),
    "htm_likelihood_update": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p]),
    "htm_likelihood_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "htm_likelihood_state_bytes": (C.c_int64, [C.c_void_p]),
    "htm_likelihood_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_likelihood_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_likelihood_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "htm_classifier_create": (C.c_int, [C.c_void_p, C.POINTER(HtmClassifierConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    "htm_classifier_destroy": (None, [C.c_void_p]),
    "htm_classifier_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p]),
    "htm_classifier_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_classifier_read_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "htm_classifier_write_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "htm_classifier_state_bytes": (C.c_int64, [C.c_void_p]),
    "htm_classifier_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_classifier_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_classifiers_create": (C.c_int, [C.c_void_p, C.POINTER(HtmClassifierConfig), C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "htm_classifiers_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                         C.c_int32, C.c_void_p, C.c_void_p]),
    "htm_classifiers_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "htm_classifiers_read_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "htm_classifiers_write_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "htm_classifiers_state_bytes": (C.c_int64, [C.c_void_p]),
    "htm_classifiers_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_classifiers_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_set_run_active_cells": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_set_group_run_active_cells": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_group_pack_columns": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "htm_group_pool_columns": (C.c_int, [C.c_void_p, HtmPoolLink, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]),
    "htm_classifiers_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "htm_knn_create": (C.c_int, [C.c_void_p, C.POINTER(HtmKnnConfig), C.POINTER(C.c_void_p)]),
    "htm_knn_destroy": (None, [C.c_void_p]),
    "htm_knn_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "htm_knn_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p]),
    "htm_knn_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "htm_knn_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_knn_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_knn_info": (C.c_int, [C.c_void_p, C.POINTER(HtmKnnInfo)]),
    "htm_knns_create": (C.c_int, [C.c_void_p, C.POINTER(HtmKnnConfig), C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "htm_knns_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "htm_knns_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    "htm_knns_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "htm_knns_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_knns_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "htm_knns_info": (C.c_int, [C.c_void_p, C.POINTER(HtmKnnsInfo), C.c_void_p]),
    "htm_knns_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HtmScalarField), C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
}

# The HIP runtime calls the binding makes itself -- the device buffers of run(record=...) -- resolved through the library's own
# handle, i.e. in exactly the runtime the library is linked against (a second runtime in the process, such as one a torch
# wheel bundles, would be a different device context: its pointers are not the library's).
HIP_EXPORTS = {
    "hipSetDevice": (C.c_int, [C.c_int]),
    "hipMalloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "hipFree": (C.c_int, [C.c_void_p]),
    "hipMemcpy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "hipGetErrorString": (C.c_char_p, [C.c_int]),
    "hipStreamCreateWithFlags": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint]),
    "hipStreamDestroy": (C.c_int, [C.c_void_p]),
}
HIP_MEMCPY_HOST_TO_DEVICE = 1
HIP_MEMCPY_DEVICE_TO_HOST = 2

_lib = None


def load():
    """Load the shared library once; raise ImportError (never fall back) if that fails."""
    global _lib
    if _lib is not None:
        return _lib
    # BITHTM_LIBRARY: another build of THIS library (same sources, same C ABI) -- the sanitizer build of its host code that
    # tests/test_host_sanitizers.py links against a HIP runtime made of host memory.  Not a fallback: unset, a missing
    # library is an error.
    path = os.environ.get("BITHTM_LIBRARY") or LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: the HIP extension is not built. Run `python -m bithtm_amd.build` "
            "(or __graft_entry__.build()). There is no CPU fallback.")
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise ImportError(f"cannot load {path}: {e}. There is no CPU fallback.") from e
    for name, (restype, argtypes) in list(EXPORTS.items()) + list(HIP_EXPORTS.items()):
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.htm_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.htm_abi_version()} != {ABI_VERSION}; rebuild")
    _lib = lib
    return lib
