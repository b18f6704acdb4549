"""One device engine = one handle of the C ABI (include/bithtm_hip.h): all device state of one
SpatialPooler and / or TemporalMemory.  Host logic only; every computation is a HIP kernel."""

import contextlib
import ctypes as C

import numpy as np

from . import _lib as L


class HtmError(RuntimeError):
    pass


class CapacityError(HtmError):
    """The fixed-capacity segment pool or a segment's synapse slots are exhausted."""


def pack_bits(bits, words):
    """bool[I] -> uint32[words], bit i of the input = bit (i & 31) of word (i >> 5).  An input that is packed already (a
    contiguous uint32 array of `words` words: a caller that keeps its inputs packed, or packs them once) goes through as it is."""
    if type(bits) is np.ndarray and bits.dtype == np.uint32 and bits.ndim == 1 and bits.size == words and bits.flags.c_contiguous:
        return bits
    bits = np.asarray(bits)
    if bits.dtype != np.bool_:
        bits = bits.astype(np.bool_)
    packed = np.packbits(bits, bitorder="little")
    if packed.size == words * 4:                    # (an input_dim that fills its words: no padding to add)
        return packed.view(np.uint32)
    out = np.zeros(words * 4, dtype=np.uint8)
    out[:len(packed)] = packed
    return out.view(np.uint32)


# run(record=...): the per-step fields htm_run_recorded can write, and the counts of one htm_step_record in its order
# ("predicted_value": the votes of "predicted_input" decoded on the device per field of an encoder -- with an `encoder=` only)
RECORD_FIELDS = ("counters", "active_column", "column_prediction", "predicted_input", "predicted_value")
RECORD_COUNTERS = tuple(name for name, _ in L.HtmStepRecord._fields_)
# SpatialPooler.run(record=...): the per-step fields htm_sp_run can write, in the order of htm_sp_run_record, with the dtype of
# each and its 32-bit words per value
SP_RECORD_FIELDS = ("active_column", "active_overlap", "active_boosted")
SP_RECORD_TYPES = {"active_column": (np.int32, 1), "active_overlap": (np.int32, 1), "active_boosted": (np.float64, 2)}


def words_per_column(cell_dim):
    """32-bit words of cells per column in the device's dense cell arrays: one up to 32 cells, two up to 64."""
    return max(1, -(-int(cell_dim) // 32))


def words_to_bool(words, cell_dim):
    """uint32[C * W] (W = words_per_column(cell_dim) words per column, side by side) -> bool[C, K]."""
    w = words_per_column(cell_dim)
    words = np.ascontiguousarray(words, dtype="<u4").reshape(-1, w)
    # (bit b of a little-endian word is bit b & 7 of its byte b >> 3: unpackbits in little bit order lays a column's cells out in
    # order -- a fifth of the time of shifting every word by 0..31)
    bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :cell_dim].view(np.bool_) if cell_dim == 32 * w else np.ascontiguousarray(bits[:, :cell_dim]).view(np.bool_)


def bool_to_words(mat):
    """bool[C, K] -> uint32[C * W]."""
    mat = np.asarray(mat, dtype=np.bool_)
    C, K = mat.shape
    w = words_per_column(K)
    padded = np.zeros((C, 32 * w), dtype=np.uint32)
    padded[:, :K] = mat
    return (padded.reshape(C, w, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2).astype(np.uint32).reshape(-1)


def check_lists(lists, column_dim):
    """The bank of active-column lists a stand-alone Temporal Memory run reads (htm_tm_run): int32 [n_rows, n], contiguous, after
    the host-side check that is made once per bank -- two dimensions with at least one row and one column, every id in
    [0, column_dim), no id twice in a row, n at most column_dim -- else ValueError."""
    a = np.asarray(lists)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"active-column lists: an integer array [n_rows, n] with at least one row and one column, got shape {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"active-column lists: integer column ids, got dtype {a.dtype}")
    if a.shape[1] > column_dim:
        raise ValueError(f"active-column lists: {a.shape[1]} ids per row, but there are only {column_dim} columns")
    if a.min() < 0 or a.max() >= column_dim:
        row = int(np.argwhere((a < 0) | (a >= column_dim))[0][0])
        raise ValueError(f"active-column lists: row {row} has a column id outside [0, {column_dim})")
    ordered = np.sort(a, axis=1)
    twice = (ordered[:, 1:] == ordered[:, :-1]).any(axis=1)
    if twice.any():
        raise ValueError(f"active-column lists: row {int(np.flatnonzero(twice)[0])} lists a column twice")
    return np.ascontiguousarray(a, dtype=np.int32)


def run_flags(use_graph=True, pipeline=True, continuing=False):
    """The flag word of the run calls (include/bithtm_hip.h: HTM_RUN_GRAPH, HTM_RUN_NO_PIPELINE, HTM_RUN_CONTINUE)."""
    return (1 if use_graph else 0) | (0 if pipeline else 2) | (4 if continuing else 0)


_NOTHING_TO_SET = contextlib.nullcontext()         # Engine.this_call: the block of a call without settings of its own


class Engine:
    LIST_BANKS = 8                                  # upload_lists: device banks of lists kept per engine
    VALUE_BANKS = 8                                 # encoded_bank: encoded banks (and their values) kept per engine
    POOL_LOOK_EVERY = 128                           # pool_look: host-fed steps between two looks at a growing pool

    def __init__(self, input_dim, column_dim, cell_dim, active_columns, proximal=None, boosting=None,
                 distal=None, seed=0, device=0, stream=None, shard_rank=0, shard_world=1, stream_owner=None):
        self.lib = L.load()
        self.input_dim = int(input_dim) if proximal is not None else 0
        self.column_dim = int(column_dim)
        self.cell_dim = int(cell_dim) if distal is not None else 0
        self.active_columns = int(active_columns)
        self.has_sp = proximal is not None
        self.has_tm = distal is not None
        self.cell_words = self.column_dim * words_per_column(self.cell_dim)     # length of the dense cell-word fields (F_CELL_*, F_WINNER_WORDS)
        cfg = L.HtmConfig()
        cfg.struct_bytes = C.sizeof(L.HtmConfig)
        cfg.device = device
        cfg.input_dim, cfg.column_dim, cfg.cell_dim = self.input_dim, self.column_dim, self.cell_dim
        cfg.active_columns = self.active_columns
        cfg.enable_sp, cfg.enable_tm = int(self.has_sp), int(self.has_tm)
        if self.has_sp:
            inc, dec = proximal.permanence_increment, proximal.permanence_decrement
            cfg.sp_permanence_threshold = proximal.permanence_threshold
            cfg.sp_delta_on = 1.0 * (inc + dec) - dec                 # projections.py:24
            cfg.sp_delta_off = 0.0 * (inc + dec) - dec
            density = boosting.active_outputs / boosting.output_dim     # regularizations.py:9
            cfg.boost_coefficient = np.float32(-(boosting.intensity / density))   # :16
            cfg.duty_momentum = np.float32(boosting.momentum)                     # :20
            cfg.duty_increment = np.float32(1.0 - boosting.momentum)              # :21
        if self.has_tm:
            a, b = distal.permanence_increment, -distal.permanence_decrement      # projections.py:287
            pa, pb = -distal.permanence_punishment, 0.0                           # :292
            cfg.tm_learn_active, cfg.tm_learn_inactive = 1.0 * (a - b) + b, 0.0 * (a - b) + b   # :102
            cfg.tm_punish_active, cfg.tm_punish_inactive = 1.0 * (pa - pb) + pb, 0.0 * (pa - pb) + pb
            cfg.tm_learn_prune, cfg.tm_punish_prune = int(min(a, b) < 0), int(min(pa, pb) < 0)   # :105
            cfg.tm_permanence_initial = np.float32(distal.permanence_initial)
            cfg.tm_permanence_threshold = np.float32(distal.permanence_threshold)
            cfg.segment_activation_threshold = distal.segment_activation_threshold
            cfg.segment_matching_threshold = distal.segment_matching_threshold
            cfg.segment_sampling_synapses = distal.segment_sampling_synapses
            cap = distal.segment_capacity
            cfg.segment_capacity = int(cap) if cap is not None else max(4096, 512 * self.active_columns)
            cfg.segment_slots = int(distal.segment_slots)
            cfg.segment_capacity_local = int(getattr(distal, "segment_capacity_local", None) or 0)
        cfg.seed = int(seed) & 0xFFFFFFFF
        cfg.shard_rank, cfg.shard_world = int(shard_rank), int(shard_world)
        # stream: None = a private stream; "default" = the device's default stream; else a hipStream_t of the caller
        cfg.use_caller_stream = int(stream is not None)
        cfg.stream = stream if (stream and stream != "default") else None
        self.shard_rank, self.shard_world = int(shard_rank), max(int(shard_world), 1)
        per = self.column_dim // self.shard_world
        self.column_range = (self.shard_rank * per, (self.shard_rank + 1) * per)
        self.segment_capacity, self.segment_slots = cfg.segment_capacity, cfg.segment_slots
        self.seed = cfg.seed
        handle = C.c_void_p()
        rc = self.lib.htm_create(C.byref(cfg), C.byref(handle))
        if rc != 0:
            raise HtmError(f"htm_create failed ({rc}): {self.lib.htm_last_error(None).decode()}")
        self.h = handle
        self.steps = 0
        self.device = int(device)
        # (a default-sized pool grows like the reference's arrays: pool_look)
        self._host_state(auto_grow=self.has_tm and distal.segment_capacity is None, stream_owner=stream_owner)
        if self.has_sp:
            c0, c1 = self.column_range          # a sharded handle only ever reads its own rows
            self.set_permanence(proximal.permanence[c0:c1] if hasattr(type(proximal), "permanence") else proximal._permanence[c0:c1],
                                row_begin=c0)
            self.words = self.info().words_per_row

    # the parent's attributes an inference view shares (shape, configuration, step index; not its buffers)
    _VIEW_ATTRS = ("lib", "input_dim", "column_dim", "cell_dim", "active_columns", "has_sp", "has_tm", "cell_words", "shard_rank",
                   "shard_world", "column_range", "segment_capacity", "segment_slots", "seed", "device", "words", "steps")

    def _host_state(self, auto_grow, stream_owner):
        """The host-side state of one handle, all of it: what __init__ and view_of start with."""
        self._record_bufs = {}                      # run(record=...): device buffers kept for the next recorded call
        self._reset_bufs = {}                       # run(resets=...): packed reset bits per content
        self._list_bufs = {}                        # upload_lists: device banks of active-column lists per content
        self._value_bufs = {}                       # encoded_bank: (device values, device bank) per encoder and content
        self._live_states = []                      # weak references to the States of the current step (networks.retire_states)
        self._auto_grow = auto_grow                 # pool_look: the pool's size was left to the library
        self._since_check = self.POOL_LOOK_EVERY    # host-fed steps since the last look (the first step looks)
        self._free_segments = 0                     # what the last look found, and the sizes to grow to if it asked for growth
        self._grow_to = (None, None)
        self._epsilon = 1e-8                        # use_epsilon: what the handle compares with (htm_create's default)
        self._stream_owner = stream_owner           # (the object whose stream `stream=` named: kept alive with the engine)

    def carry_from(self, old):
        """The host state a re-created engine keeps from the one it replaces (grow_pool): whether its pool grows."""
        self._auto_grow = old._auto_grow

    @classmethod
    def view_of(cls, parent):
        """An inference view of `parent` (htm_create_view): a handle that aliases the parent's weights and owns its stream
        state, starting as the parent would be after reset().  It steps with learning=False only."""
        v = cls.__new__(cls)
        for a in cls._VIEW_ATTRS:
            if a in parent.__dict__:
                setattr(v, a, parent.__dict__[a])
        handle = C.c_void_p()
        rc = v.lib.htm_create_view(parent.h, C.byref(handle))
        if rc != 0:
            raise HtmError(f"htm_create_view failed ({rc}): {v.lib.htm_last_error(None).decode()}")
        v.h = handle
        v._host_state(auto_grow=False, stream_owner=parent._stream_owner)     # (the parent's pool grows; a view never adds a segment)
        v.is_view = True
        return v

    def view_sync(self, source):
        """This view's stream state becomes that of the engine `source` -- its parent's, or another view's of the same parent --
        on the device (htm_view_sync: one launch on the shared stream, no wait); the step index comes with it."""
        self._check(self.lib.htm_view_sync(self.h, source.h), "htm_view_sync")
        self.steps = source.steps

    def bank_rows(self, device_bank, bank_rows, first_step, n, device_dst):
        """device_dst row r = row (first_step + r) % bank_rows of a device bank, r < n (htm_bank_rows): enqueued, no wait."""
        self._check(self.lib.htm_bank_rows(self.h, C.c_void_p(device_bank), int(bank_rows), int(first_step), int(n), C.c_void_p(device_dst)),
                    "htm_bank_rows")

    def device_bytes(self):
        """Device bytes this handle allocated itself (a view does not count the weights it shares: htm_device_bytes)."""
        return int(self._check(self.lib.htm_device_bytes(self.h), "htm_device_bytes"))

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            self.lib.htm_destroy(h)             # (synchronises its stream: the record buffers are idle after it)
        for ptr, _ in getattr(self, "_record_bufs", {}).values():
            self.lib.hipFree(ptr)
        for ptr in list(getattr(self, "_reset_bufs", {}).values()) + list(getattr(self, "_list_bufs", {}).values()):
            self.lib.hipFree(ptr)
        for pair in getattr(self, "_value_bufs", {}).values():
            for ptr in pair:
                self.lib.hipFree(ptr)

    # ---- plumbing
    def _check(self, rc, what):
        if rc < 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.htm_last_error(self.h).decode()}")
        return rc

    def info(self):
        """htm_info of the last completed step (does not raise on a capacity overflow: see
        check_capacity)."""
        out = L.HtmInfo()
        rc = self.lib.htm_get_info(self.h, C.byref(out))
        if rc != -3:                      # HTM_ERR_CAPACITY still fills `out`
            self._check(rc, "htm_get_info")
        return out

    def check_capacity(self):
        info = self.info()
        if info.capacity_error:
            raise CapacityError(self.lib.htm_last_error(self.h).decode())
        return info

    def pool_look(self, per_step, force=False):
        """Pools whose size the user did not fix (`segment_capacity=None`) follow the reference's growing arrays
        (utils.py:113-135): every POOL_LOOK_EVERY host-fed steps (`force`: now -- between two device-side batches, never inside
        one) the engine is asked how full it is (a synchronisation and a read-back: not more often), and True comes back -- with
        the sizes to grow to in _grow_to and the free segments in _free_segments -- when the free segments would not last another
        POOL_LOOK_EVERY steps at `per_step` new segments each (every active column bursting), or a segment has filled three
        quarters of its slots."""
        if not self._auto_grow or not self.has_tm:
            return False
        every = self.POOL_LOOK_EVERY
        self._since_check += 1
        if self._since_check < every and not force:
            return False
        self._since_check = 0
        info = self.check_capacity()
        self._free_segments = self.segment_capacity - info.segments
        capacity = slots = None
        if self._free_segments < (every + 1) * per_step:
            capacity = max(2 * self.segment_capacity, info.segments + 4 * (every + 1) * per_step)
        if info.segments and self.segment_slots < 512:
            nsyn = self.read(L.F_SEG_NSYN, np.int32, info.local_segments)
            if int(nsyn.max(initial=0)) > 3 * self.segment_slots // 4:      # (a segment gains at most one sample of synapses per step)
                slots = min(512, 2 * self.segment_slots)
        self._grow_to = (capacity, slots)
        return capacity is not None or slots is not None

    def sync(self):
        self._check(self.lib.htm_sync(self.h), "htm_sync")

    def planes_check(self):
        """(mismatches, plane_steps): the bytes of the mask's byte planes that differ from the connected mask, compared on the
        device (-1: the handle keeps no planes -- a shard), and the steps so far whose overlap was counted from the planes."""
        out = (C.c_int64 * 2)()
        self._check(self.lib.htm_sp_planes_check(self.h, out), "htm_sp_planes_check")
        return int(out[0]), int(out[1])

    def stream_handle(self):
        """The hipStream_t this engine enqueues on (an integer; 0 = the default stream)."""
        out = C.c_void_p()
        self._check(self.lib.htm_get_stream(self.h, C.byref(out)), "htm_get_stream")
        return out.value or 0

    def shard_run(self, device_bank, n_inputs, n_steps, learning=True, use_graph=True, pipeline=True):
        """n_steps column-sharded timesteps, the exchange (RCCL) and the loop inside the library (htm_shard_run)."""
        self._check(self.lib.htm_shard_run(self.h, C.c_void_p(device_bank), int(n_inputs), int(n_steps), int(bool(learning)),
                                           run_flags(use_graph, pipeline)), "htm_shard_run")
        self.steps += n_steps

    def import_prev_state(self, prediction, activation, winner_flat, distal):
        """TemporalMemory.process(prev_state=X) (networks.py:92-93): X's fields become the handle's "previous step" --
        cell predictions and activations (bool [C, K]), winner cells (flat ids, or None), the PredictiveProjection.State
        (or None) -- while the segment store and the step index stay what they are."""
        K = self.cell_dim
        S = self.info().segments
        self._check(self.lib.htm_import_begin(self.h, -1), "htm_import_begin")     # HTM_IMPORT_PREV_STATE: store, step index, flags stay
        self.write(L.F_CELL_PREDICTION, bool_to_words(np.asarray(prediction).reshape(self.column_dim, K)), np.uint32)
        self.write(L.F_CELL_ACTIVATION, bool_to_words(np.asarray(activation).reshape(self.column_dim, K)), np.uint32)
        winners = np.zeros(0, np.int32) if winner_flat is None else np.asarray(winner_flat, dtype=np.int32)
        self.write(L.F_WINNER_CELL, winners, np.int32)
        M = 0
        if distal is not None:
            seg = np.asarray(distal.matching_segment, dtype=np.int32)
            M = len(seg)
            pot = np.zeros(S, dtype=np.int64)              # (the store may have grown since X: potentials of newer segments are not used)
            old = np.asarray(distal.segment_potential, dtype=np.int64)[:S]
            pot[:len(old)] = old
            minfo = (pot[seg].astype(np.uint32) | (np.asarray(distal.matching_segment_activation).astype(np.uint32) << 12)
                     | (np.asarray(distal.matching_segment_active).astype(np.uint32) << 31))
            self.write(L.F_SEG_POTENTIAL, pot, np.int32)
            self.write(L.F_MATCH_SEGMENT, seg, np.int32)
            self.write(L.F_MATCH_INFO, minfo, np.uint32)
            self.write(L.F_MATCH_JITTER, np.asarray(distal.matching_segment_jittered_potential, dtype=np.float32), np.float32)
            self.write(L.F_CELL_MAX_JITTER, np.asarray(distal.max_jittered_potential, dtype=np.float32).view(np.uint32), np.uint32)
        self._check(self.lib.htm_import_commit(self.h, int(S), int(M), len(winners), int(distal is not None), int(winner_flat is not None)),
                    "htm_import_commit")

    def reset(self):
        """A sequence reset (htm_reset): the previous step becomes TemporalMemory.get_empty_state() on the device -- what
        import_prev_state of the empty state leaves, without the host copies."""
        self._check(self.lib.htm_reset(self.h), "htm_reset")

    def upload_resets(self, resets):
        """bool[n] (reset before every step that reads bank row r) -> device address of the packed bits htm_set_run_resets
        takes.  Kept by the engine per content (freed with it)."""
        bits = np.ascontiguousarray(np.asarray(resets, dtype=np.bool_).ravel())
        key = (bits.size, bits.tobytes())
        bufs = self._reset_bufs
        if key not in bufs:
            words = np.zeros((bits.size + 31) // 32 * 4, dtype=np.uint8)
            pb = np.packbits(bits, bitorder="little")
            words[:pb.size] = pb
            bufs[key] = self.device_buffer(words.size, words)
        return bufs[key]

    def set_run_resets(self, device_bits, n_inputs):
        """Reset bits of the later run() / prepare() calls on banks of n_inputs rows (htm_set_run_resets); None clears them."""
        self._check(self.lib.htm_set_run_resets(self.h, C.c_void_p(device_bits) if device_bits else None, int(n_inputs)),
                    "htm_set_run_resets")

    def set_epsilon(self, epsilon):
        """TemporalMemory.process(epsilon=) (networks.py:91): 0 < epsilon <= 1, compared as float32; stays until set again."""
        self._check(self.lib.htm_set_epsilon(self.h, C.c_float(float(epsilon))), "htm_set_epsilon")

    def use_epsilon(self, epsilon):
        """The steps that follow compare with `epsilon`: set_epsilon, unless the last use_epsilon asked for the same."""
        if self._epsilon != epsilon:
            self.set_epsilon(epsilon)
            self._epsilon = epsilon

    def this_call(self, resets=None, n_inputs=0, feedback=None, votes=None, cells=None):
        """Settings that hold for the calls inside the block only, set in this order and cleared in reverse on the way out,
        whatever happens inside: `resets` (set_run_resets on banks of n_inputs rows), `feedback` (set_run_feedback's
        arguments), `votes` (set_run_predicted_input), `cells` (set_run_active_cells).  None: left alone -- and with nothing to set, the plain run()'s case,
        a block that costs nothing (streamed callers make a run() call per chunk)."""
        if resets is None and feedback is None and votes is None and cells is None:
            return _NOTHING_TO_SET
        return self._settings(resets, n_inputs, feedback, votes, cells)

    @contextlib.contextmanager
    def _settings(self, resets, n_inputs, feedback, votes, cells=None):
        undo = []
        try:
            if resets is not None:
                self.set_run_resets(resets, n_inputs)
                undo.append(lambda: self.set_run_resets(None, 0))
            if feedback is not None:
                self.set_run_feedback(*feedback)
                undo.append(lambda: self.set_run_feedback(None))
            if votes is not None:
                self.set_run_predicted_input(votes)
                undo.append(lambda: self.set_run_predicted_input(None))
            if cells is not None:
                self.set_run_active_cells(cells)
                undo.append(lambda: self.set_run_active_cells(None))
            yield
        finally:
            for clear in reversed(undo):
                clear()

    def read(self, field, dtype, count):
        out = np.empty(int(count), dtype=dtype)
        n = self._check(self.lib.htm_read(self.h, field, out.ctypes.data_as(C.c_void_p), out.size), "htm_read")
        return out[:n]

    def read_rows(self, field, dtype, row_begin, row_count):
        """Rows [row_begin, row_begin + row_count) of a per-segment field (htm_read_rows)."""
        per = self.segment_slots if field in (L.F_SEG_PRESYN, L.F_SEG_PERM) else 1
        out = np.empty(int(row_count) * per, dtype=dtype)
        n = self._check(self.lib.htm_read_rows(self.h, field, int(row_begin), int(row_count), out.ctypes.data_as(C.c_void_p), out.size),
                        "htm_read_rows")
        return out[:n].reshape(int(row_count), per) if per > 1 else out[:n]

    def write(self, field, array, dtype):
        a = np.ascontiguousarray(array, dtype=dtype)
        self._check(self.lib.htm_write(self.h, field, a.ctypes.data_as(C.c_void_p), a.size), "htm_write")

    # ---- SP state
    def set_permanence(self, perm, row_begin=0):
        perm = np.ascontiguousarray(perm, dtype=np.float64)
        assert perm.ndim == 2 and perm.shape[1] == self.input_dim
        self._check(self.lib.htm_sp_set_permanence(self.h, perm.ctypes.data_as(C.c_void_p), row_begin, perm.shape[0]),
                    "htm_sp_set_permanence")

    def get_permanence(self, row_begin=0, row_count=None):
        row_count = self.column_dim - row_begin if row_count is None else row_count
        out = np.empty((row_count, self.input_dim), dtype=np.float64)
        self._check(self.lib.htm_sp_get_permanence(self.h, out.ctypes.data_as(C.c_void_p), row_begin, row_count),
                    "htm_sp_get_permanence")
        return out

    def read_duty_cycle(self):
        return self.read(L.F_DUTY_CYCLE, np.float32, self.column_dim)

    # ---- stepping
    def step(self, input_bits, learning=True):
        packed = pack_bits(input_bits, self.words)
        rc = self.lib.htm_step(self.h, packed.ctypes.data, 1 if learning else 0)
        if rc < 0:
            self._check(rc, "htm_step")
        self.steps += 1

    def sp_step(self, input_bits, learning=True):
        packed = pack_bits(input_bits, self.words)
        self._check(self.lib.htm_sp_step(self.h, packed.ctypes.data_as(C.c_void_p), int(bool(learning))), "htm_sp_step")
        self.steps += 1

    def sp_phase(self, phase, data=None, dtype=None):
        """One phase of SpatialPooler.process on the current timestep (htm_sp_phase, include/bithtm_hip.h)."""
        if data is None:
            rc = self.lib.htm_sp_phase(self.h, int(phase), None, 0)
        elif phase in (L.SP_OVERLAP, L.SP_LEARN):
            packed = pack_bits(data, self.words)
            rc = self.lib.htm_sp_phase(self.h, int(phase), packed.ctypes.data_as(C.c_void_p), packed.size)
        else:
            a = np.ascontiguousarray(data, dtype=dtype)
            rc = self.lib.htm_sp_phase(self.h, int(phase), a.ctypes.data_as(C.c_void_p), a.size)
        self._check(rc, "htm_sp_phase")
        if phase == L.SP_COMMIT:
            self.steps += 1

    def tm_step(self, active_column, learning=True, return_winner_cell=True):
        cols = np.ascontiguousarray(active_column, dtype=np.int32)
        self._check(self.lib.htm_tm_step(self.h, cols.ctypes.data_as(C.c_void_p), cols.size, int(bool(learning)),
                                         int(bool(return_winner_cell))), "htm_tm_step")
        self.steps += 1

    def tm_update(self, columns, winner_words, unaccounted_words, punish_words=None):
        """PredictiveProjection.update on its own (htm_tm_update, include/bithtm_hip.h)."""
        cols = np.ascontiguousarray(columns, dtype=np.int32)
        ww = np.ascontiguousarray(winner_words, dtype=np.uint32)
        uw = np.ascontiguousarray(unaccounted_words, dtype=np.uint32)
        pw = None if punish_words is None else np.ascontiguousarray(punish_words, dtype=np.uint32)
        self._check(self.lib.htm_tm_update(self.h, cols.ctypes.data_as(C.c_void_p), ww.ctypes.data_as(C.c_void_p), uw.ctypes.data_as(C.c_void_p),
                                           cols.size, None if pw is None else pw.ctypes.data_as(C.c_void_p)), "htm_tm_update")

    def tm_scan(self, active_words):
        """PredictiveProjection.process on its own (htm_tm_scan); closes the timestep."""
        aw = np.ascontiguousarray(active_words, dtype=np.uint32)
        assert aw.size == self.cell_words
        self._check(self.lib.htm_tm_scan(self.h, aw.ctypes.data_as(C.c_void_p)), "htm_tm_scan")
        self.steps += 1

    def upload_lists(self, lists, check=True):
        """int32 [n_rows, n] active-column lists -> device address of the bank tm_run reads.  Checked on the host once per bank
        (check_lists: ValueError; check=False uploads the rows as they are -- the device checks every row it reads all the same,
        htm_tm_run) and kept by the engine per content: the same array again costs no upload, and the LIST_BANKS most recent
        banks stay (freed with the engine)."""
        a = check_lists(lists, self.column_dim) if check else np.ascontiguousarray(lists, dtype=np.int32)
        key = (a.shape, a.tobytes())
        bufs = self._list_bufs
        if key in bufs:
            bufs[key] = bufs.pop(key)               # (most recent last)
            return bufs[key]
        if len(bufs) >= self.LIST_BANKS:
            self.sync()                             # (a run that reads the oldest bank may still be queued)
            self.lib.hipFree(bufs.pop(next(iter(bufs))))
        bufs[key] = self.device_buffer(a.nbytes, a, at_least=4)
        return bufs[key]

    def tm_run(self, device_lists, n_rows, n, n_steps, learning=True, use_graph=True, record=None, resets=None, check=True):
        """n_steps stand-alone Temporal Memory steps over a device bank of lists (upload_lists: n_rows rows of n ids), the loop
        on the device (htm_tm_run).  `record`: None, or fields of RECORD_FIELDS other than "predicted_input": the call then
        returns {field: numpy array over the steps} as _run does -- "active_column" int32[n_steps, active_columns], each row
        the step's sorted list in its first n slots and -1 behind them.  `resets`: None, or the device address of reset bits
        for the bank's rows (upload_resets), set for this call only.  `check`: wait for the call and raise CapacityError if
        it set a sticky flag -- an overflowed pool, or a row the device found invalid (check_capacity)."""
        fields = () if record is None else self._record_fields(record, RECORD_FIELDS[:3])
        n_steps = int(n_steps)
        rec = L.HtmRunRecord()
        self._record_args(fields, n_steps, rec)
        with self.this_call(resets, n_rows):
            self._check(self.lib.htm_tm_run(self.h, C.c_void_p(device_lists), int(n_rows), int(n), n_steps, int(bool(learning)),
                                            run_flags(use_graph), C.byref(rec) if fields else None), "htm_tm_run")
        self.steps += n_steps
        if check:
            self.check_capacity()
        return None if record is None else self._records_read(fields, n_steps, sync=True)

    def sp_run(self, device_bank, n_inputs, n_steps, learning=True, use_graph=True, record=None):
        """n_steps stand-alone Spatial Pooler steps over a device bank (upload_bank: n_inputs rows), the loop on the device
        (htm_sp_run).  `record`: None, or fields of SP_RECORD_FIELDS: the call then returns {field: numpy array
        [n_steps, active_columns]} -- int32 columns (ascending), int32 overlaps, float64 boosted overlaps of each step's winners
        -- read back after one synchronisation."""
        fields = () if record is None else self._record_fields(record, SP_RECORD_FIELDS)
        n_steps, k = int(n_steps), self.active_columns
        rec = L.HtmSpRunRecord()
        rec.struct_bytes = C.sizeof(L.HtmSpRunRecord)
        for f in fields:
            setattr(rec, f, self._record_buffer("sp_" + f, max(n_steps, 1) * k * SP_RECORD_TYPES[f][1]))
        self._check(self.lib.htm_sp_run(self.h, C.c_void_p(device_bank), int(n_inputs), n_steps, int(bool(learning)),
                                        run_flags(use_graph), C.byref(rec) if fields else None), "htm_sp_run")
        self.steps += max(n_steps, 0)
        if record is None:
            return None
        self.sync()
        out = {}
        for f in fields:
            dtype, words = SP_RECORD_TYPES[f]
            out[f] = self._record_read("sp_" + f, n_steps * k * words, np.uint32).view(dtype).reshape(n_steps, k)
        return out

    def upload_bank(self, inputs):
        """bool[n, I] -> device address of the packed bank htm_run reads."""
        inputs = np.asarray(inputs, dtype=np.bool_)
        n = inputs.shape[0]
        words = (self.input_dim + 31) // 32
        packed = np.zeros((n, words * 4), dtype=np.uint8)
        pb = np.packbits(inputs, axis=1, bitorder="little")
        packed[:, :pb.shape[1]] = pb
        ptr = C.c_void_p()
        self._check(self.lib.htm_bank_upload(self.h, packed.ctypes.data_as(C.c_void_p), n, C.byref(ptr)), "htm_bank_upload")
        return ptr.value

    def run(self, device_bank, n_inputs, n_steps, learning=True, use_graph=True, pipeline=True, continuing=False, record=None,
            resets=None, encoder=None, likelihood=None, classifier=None, knn=None):
        """`resets`: None, or the device address of reset bits for this bank (upload_resets): a sequence reset before every
        step that reads a row whose bit is set (htm_set_run_resets, set for this call only).  `encoder`: the ScalarEncoder a
        "predicted_value" record decodes with."""
        with _NOTHING_TO_SET if resets is None else self.this_call(resets, n_inputs):
            return self._run(device_bank, n_inputs, n_steps, learning, use_graph, pipeline, continuing, record, encoder, likelihood, classifier, knn)

    def _run(self, device_bank, n_inputs, n_steps, learning=True, use_graph=True, pipeline=True, continuing=False, record=None,
             encoder=None, likelihood=None, classifier=None, knn=None):
        """`continuing`: the next call is another run() on the same bank (HTM_RUN_CONTINUE, include/bithtm_hip.h).
        `record`: None, or the fields of a per-step record to keep (RECORD_FIELDS): the call then goes to htm_run_recorded and
        returns {field: numpy array over the n_steps steps} -- "counters" int32[n, 8] (htm_step_record, RECORD_COUNTERS order),
        "active_column" int32[n, k], "column_prediction" uint32[n, ceil(C / 32)], "predicted_input" int32[n, input_dim] (the
        votes of htm_set_run_predicted_input, set for this call only), "predicted_value" int32[n, 2 F] (with `encoder`: the (bucket,
        score) pairs of its F fields, decoded behind the run from the rows "predicted_input" uses, which stay on the device unless
        they were asked for too) -- read back after one synchronisation.  `likelihood` (an anomaly.AnomalyLikelihood of one stream;
        `record` has "counters"): its update over the counters' buffer is enqueued behind the run, before that synchronisation,
        and "anomaly_likelihood" float64[n] is returned beside the fields.  `classifier` (`record` is not None): {"clf": an
        sdr_classifier.SDRClassifier, "targets": device address of int32 [rows], "rows", "resets": device address of reset bits over
        those rows or None, "learn", "distribution"} -- the run leaves each step's active-cell words in the classifier's pattern
        buffer (htm_set_run_active_cells, set for this call only), the classifier's update is enqueued behind the run, before the
        synchronisation, step i reading target and reset bit (step index + i) % rows, and "classified" int32[n, H, 2] and
        "class_distribution" (int32[n, H, buckets] or None) are returned beside the fields.  `knn` (`record` is not None): {"knn": a
        knn_classifier.KNNClassifier, "labels": device address of int32 [rows] (its upload_labels), "host_labels": the same labels
        int32 [rows], "learn", "votes"} -- the KNN update over the same captured rows (the classifier's buffer when both ride on the
        run: one capture launch per step either way) is enqueued next to the classifier's, step i reading label (step index + i) %
        rows, and "knn" int32[n, 5] and "knn_votes_all" (int32[n, labels] or None) are returned beside the fields."""
        if record is None:
            self.run_into(device_bank, n_inputs, n_steps, {}, learning, use_graph, pipeline, continuing)
            return None
        fields, n = self._record_fields(record), int(n_steps)
        buffers = self._record_buffers(fields, n, encoder)
        clf = classifier["clf"] if classifier is not None and n > 0 else None
        cells, first = (clf.pairs_buffer(self, n), self.steps % classifier["rows"]) if clf is not None else (None, 0)
        near = knn["knn"] if knn is not None and n > 0 else None
        if near is not None:
            knn_first = self.steps % len(knn["host_labels"])
            near.check_room(near.stored_by(knn["host_labels"], knn_first, n, knn["learn"]))      # (refused before the run is enqueued)
            cells = near.pairs_buffer(self, n) if cells is None else cells
        self.run_into(device_bank, n_inputs, n, buffers, learning, use_graph, pipeline, continuing, cells=cells)
        self.decode_records(buffers, n, encoder)
        if likelihood is not None and n > 0:
            likelihood.enqueue(self, [buffers["counters"]], n)
        if clf is not None:
            clf.enqueue(self, cells, clf.shape[2], n, classifier["targets"], classifier["rows"], first, classifier["resets"], classifier["learn"],
                        classifier["distribution"])
        if near is not None:
            near.enqueue(self, cells, near.shape[2], n, knn["labels"], knn["host_labels"], knn_first, knn["learn"], knn["votes"])
        out = self._records_read(fields, n, sync=True, encoder=encoder)
        if likelihood is not None:
            out["anomaly_likelihood"] = likelihood.read(self, n)[0] if n > 0 else np.zeros(0, dtype=np.float64)
        if classifier is not None:
            c = classifier["clf"]
            out["classified"], out["class_distribution"] = c.read(self, n, classifier["distribution"]) if n > 0 else (
                np.zeros((0, len(c.steps), 2), np.int32), np.zeros((0, len(c.steps), c.buckets), np.int32) if classifier["distribution"] else None)
        if knn is not None:
            c = knn["knn"]
            out["knn"], out["knn_votes_all"] = c.read(self, n, knn["votes"]) if n > 0 else (
                np.zeros((0, 5), np.int32), np.zeros((0, c.labels), np.int32) if knn["votes"] else None)
        return out

    def run_into(self, device_bank, n_inputs, n_steps, buffers, learning=True, use_graph=True, pipeline=True, continuing=False, cells=None):
        """The run of _run, enqueued only: `buffers` = {record field: device address of its n_steps rows} (record_shapes() words
        per row; empty: a plain htm_run).  The records stay on the device: nothing is synchronised and nothing read back -- the
        caller orders its own work behind the engine's stream (region stacks feed "active_column" to htm_pack_columns).  `cells`: the
        device address of the rows a recorded run's steps leave their active-cell words in (set_run_active_cells, for this call only)."""
        flags, n = run_flags(use_graph, pipeline, continuing), int(n_steps)
        rec = L.HtmRunRecord()
        votes = self._record_ptrs(buffers, rec)
        with self.this_call(votes=votes, cells=cells):
            if not set(buffers) - {"predicted_input", "predicted_value"}:
                self._check(self.lib.htm_run(self.h, C.c_void_p(device_bank), int(n_inputs), n, int(bool(learning)), flags), "htm_run")
            else:
                self._check(self.lib.htm_run_recorded(self.h, C.c_void_p(device_bank), int(n_inputs), n, int(bool(learning)), flags,
                                                      C.byref(rec)), "htm_run_recorded")
        self.steps += n

    def pack_columns(self, device_lists, k, n_rows, stride, device_bank, bank_rows, first_row):
        """Bank rows of this engine from recorded active-column lists (htm_pack_columns): enqueued on its stream, no wait."""
        self._check(self.lib.htm_pack_columns(self.h, C.c_void_p(device_lists), int(k), int(n_rows), int(stride), C.c_void_p(device_bank),
                                              int(bank_rows), int(first_row)), "htm_pack_columns")

    def pool_columns(self, link, device_lists, k, device_column_prediction, n_rows, device_persistence, device_prev, device_reset_bits,
                     device_scratch, scratch_bytes, device_bank, bank_rows, first_row):
        """Bank rows of this engine from the recorded active-column lists and column predictions of n_rows windows, through a
        pooling link's state arrays on the device (htm_pool_columns; `link`: a resolved pooling.PoolingLink): enqueued on its
        stream, no wait."""
        p = L.HtmPoolLink(C.sizeof(L.HtmPoolLink), link.stride, link.active_weight, link.predicted_weight, link.decay, link.ceiling, link.union_bits, 0)
        self._check(self.lib.htm_pool_columns(self.h, p, C.c_void_p(device_lists), int(k), C.c_void_p(device_column_prediction), int(n_rows),
                                              C.c_void_p(device_persistence), C.c_void_p(device_prev),
                                              C.c_void_p(device_reset_bits) if device_reset_bits else None, C.c_void_p(device_scratch),
                                              int(scratch_bytes), C.c_void_p(device_bank), int(bank_rows), int(first_row)), "htm_pool_columns")

    @staticmethod
    def _record_fields(record, allowed=RECORD_FIELDS):
        """The fields of a `record` argument as a tuple; ValueError for one that is not in `allowed`, or for none."""
        fields = tuple(record)
        if set(fields) - set(allowed) or not fields:
            raise ValueError(f"record: fields from {allowed}, at least one (got {fields})")
        return fields

    def _record_buffers(self, fields, n, encoder=None):
        """{field: device address of the engine's own record buffer, large enough for n steps}; "predicted_value" (ValueError
        without an `encoder`) brings the rows of "predicted_input" with it: its decode launch reads them."""
        shapes = self.record_shapes(encoder)
        if "predicted_value" in fields:
            if encoder is None:
                raise ValueError('record "predicted_value" needs an encoder (run(..., encoder=))')
            fields = tuple(fields) + (("predicted_input",) if "predicted_input" not in fields else ())
        return {f: self._record_buffer(f, max(n, 1) * shapes[f][0]) for f in fields}

    def decode_records(self, buffers, n, encoder):
        """Behind a recorded run of n steps into `buffers`: the decode launch of its "predicted_value" rows (enqueued, no wait)."""
        if "predicted_value" in buffers and n > 0:
            self.decode_votes(encoder, buffers["predicted_input"], n, buffers["predicted_value"])

    def _record_args(self, fields, n, rec, encoder=None):
        """The record buffers of n steps for `fields` into `rec` (an HtmRunRecord) and, for "predicted_input", the decoding rows
        (set_run_predicted_input: the caller clears them) -> the buffers."""
        buffers = self._record_buffers(fields, n, encoder)
        votes = self._record_ptrs(buffers, rec)
        if votes is not None:
            self.set_run_predicted_input(votes)
        return buffers

    @staticmethod
    def _record_ptrs(ptrs, rec):
        """{field: device address} into `rec` -> the address of the decoding rows ("predicted_input": they are no part of the
        structure; set_run_predicted_input takes them), or None."""
        rec.struct_bytes = C.sizeof(L.HtmRunRecord)
        rec.records, rec.active_column, rec.column_prediction = (ptrs.get(f) for f in RECORD_FIELDS[:3])
        return ptrs.get("predicted_input")

    def _records_read(self, fields, n, sync=False, encoder=None):
        """{field: numpy array [n, words per step]} from the engine's own record buffers (`sync`: after waiting for the engine's
        stream, on which the records are written)."""
        if sync:
            self.sync()
        shapes = self.record_shapes(encoder)
        return {f: self._record_read(f, n * shapes[f][0], shapes[f][1]).reshape(n, shapes[f][0]) for f in fields}

    def record_shapes(self, encoder=None):
        """{record field: (int32 words per step, dtype)} of this engine's shape (and, with an encoder, of its "predicted_value")."""
        shapes = {"counters": (len(RECORD_COUNTERS), np.int32), "active_column": (self.active_columns, np.int32),
                  "column_prediction": ((self.column_dim + 31) // 32, np.uint32), "predicted_input": (self.input_dim, np.int32)}
        if encoder is not None:
            shapes["predicted_value"] = (2 * len(encoder), np.int32)
        return shapes

    def set_run_predicted_input(self, device_votes):
        """Decoding rows of the later run() calls and group calls (htm_set_run_predicted_input); None clears them."""
        self._check(self.lib.htm_set_run_predicted_input(self.h, C.c_void_p(device_votes) if device_votes else None),
                    "htm_set_run_predicted_input")

    def set_run_active_cells(self, device_pairs):
        """Pattern rows of the later recorded run() calls (htm_set_run_active_cells); None clears them."""
        self._check(self.lib.htm_set_run_active_cells(self.h, C.c_void_p(device_pairs) if device_pairs else None), "htm_set_run_active_cells")

    def predicted_input(self):
        """int32[input_dim]: the predicted-input votes of the current state (htm_predicted_input)."""
        out = np.empty(self.input_dim, dtype=np.int32)
        self._check(self.lib.htm_predicted_input(self.h, out.ctypes.data_as(C.c_void_p)), "htm_predicted_input")
        return out

    # ---- scalar streams (htm_scalar.h; encoders.py is the definition).  Raw device addresses: a caller with a device tensor of
    # its own encodes in place after ordering its stream against stream_handle()
    def upload_values(self, values):
        """float64 [n, F] -> device address of the values htm_bank_encode reads (the caller frees it: hipFree)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        return self.device_buffer(v.nbytes, v, at_least=8)

    def bank_encode(self, encoder, device_values, n_rows, device_bank, bank_rows, first_row=0):
        """Bank rows first_row .. first_row + n_rows - 1 = encoder.encode of the device values' rows (htm_bank_encode): enqueued on
        the engine's stream, no wait."""
        self._check(self.lib.htm_bank_encode(self.h, encoder.table(), len(encoder), C.c_void_p(device_values), int(n_rows),
                                             C.c_void_p(device_bank), int(bank_rows), int(first_row)), "htm_bank_encode")

    def decode_votes(self, encoder, device_votes, n_rows, device_out):
        """device_out [n_rows, F, 2] int32 = (bucket, score) per field of the device votes' rows, int32 [n_rows, input_dim]
        (htm_decode_votes): enqueued on the engine's stream, no wait."""
        self._check(self.lib.htm_decode_votes(self.h, encoder.table(), len(encoder), C.c_void_p(device_votes), int(n_rows),
                                              C.c_void_p(device_out)), "htm_decode_votes")

    def predicted_value(self, encoder):
        """(bucket int32[F], score int32[F]) of the current state's votes (htm_predicted_value): the votes stay on the device."""
        out = np.empty((len(encoder), 2), dtype=np.int32)
        self._check(self.lib.htm_predicted_value(self.h, encoder.table(), len(encoder), out.ctypes.data_as(C.c_void_p)), "htm_predicted_value")
        return out[:, 0].copy(), out[:, 1].copy()

    def encoded_bank(self, encoder, values):
        """float64 [n, F] -> device address of the bank of encoder.encode(values), encoded on the device: the values are
        uploaded (8 F bytes per row) and one launch fills the bank (enqueued).  Kept by the engine per encoder and content: the
        same values again cost nothing, and the VALUE_BANKS most recent banks stay (freed with the engine)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        key = (encoder.key(), v.shape, v.tobytes())
        bufs = self._value_bufs
        if key in bufs:
            bufs[key] = bufs.pop(key)               # (most recent last)
            return bufs[key][1]
        if len(bufs) >= self.VALUE_BANKS:
            self.sync()                             # (a run that reads the oldest bank may still be queued)
            for ptr in bufs.pop(next(iter(bufs))):
                self.lib.hipFree(ptr)
        n = v.shape[0]
        bufs[key] = pair = (self.upload_values(v), self.device_buffer(n * self.words * 4))
        self.bank_encode(encoder, pair[0], n, pair[1], n)
        return pair[1]

    def encode_votes(self, min_votes, max_bits, device_bank, bank_rows, row):
        """Row `row` of a device bank = the current state's votes encoded (htm_encode_votes): enqueued on the engine's stream, no
        wait."""
        self._check(self.lib.htm_encode_votes(self.h, int(min_votes), int(max_bits), C.c_void_p(device_bank), int(bank_rows), int(row)),
                    "htm_encode_votes")

    def set_run_feedback(self, device_bank, n_inputs=0, min_votes=1, max_bits=0):
        """Later run() calls and group calls on this bank write each step's encoded votes into the row the next step reads
        (htm_set_run_feedback); None clears it."""
        self._check(self.lib.htm_set_run_feedback(self.h, C.c_void_p(device_bank) if device_bank else None, int(n_inputs), int(min_votes),
                                                  int(max_bits)), "htm_set_run_feedback")

    def zero_bank(self, rows):
        """Device address of a handle-owned bank of `rows` all-zero rows (htm_bank_upload)."""
        ptr = C.c_void_p()
        zeros = np.zeros((int(rows), (self.input_dim + 31) // 32), dtype=np.uint32)
        self._check(self.lib.htm_bank_upload(self.h, zeros.ctypes.data_as(C.c_void_p), int(rows), C.byref(ptr)), "htm_bank_upload")
        return ptr.value

    def zero_resets(self, rows):
        """Device address of a handle-owned array of reset bits for `rows` bank rows, all clear (freed with the handle)."""
        words = (int(rows) + 31) // 32
        return self.zero_bank((words + self.words - 1) // self.words)       # (whole bank rows of zeros: at least `words` words)

    def bank_noise(self, src_bank, n_src, dst_bank, n_dst, first_step, n_rows, seed, threshold24, src_resets=None, dst_resets=None):
        """Ring rows of the steps first_step .. first_step + n_rows - 1: dst row (step % n_dst) = src row (step % n_src) ^ the
        keyed flips of that step (htm_bank_noise; networks.flip_noise is the definition), and with the two reset arrays the
        ring's reset bits from the source's.  Enqueued on the engine's stream, no wait."""
        self._check(self.lib.htm_bank_noise(self.h, C.c_void_p(src_bank), int(n_src), C.c_void_p(dst_bank), int(n_dst),
                                            int(first_step) & 0xFFFFFFFF, int(n_rows), int(seed) & 0xFFFFFFFF, int(threshold24),
                                            C.c_void_p(src_resets) if src_resets else None, C.c_void_p(dst_resets) if dst_resets else None),
                    "htm_bank_noise")

    def read_resets(self, device_bits, rows):
        """bool[rows]: reset bits in device memory (upload_resets' layout), after a synchronisation."""
        self.sync()
        out = np.empty((int(rows) + 31) // 32, dtype=np.uint32)
        self._hip_check(self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(device_bits), out.nbytes, L.HIP_MEMCPY_DEVICE_TO_HOST),
                        "hipMemcpy")
        return np.unpackbits(out.view(np.uint8), bitorder="little")[:int(rows)].astype(np.bool_)

    def read_bank(self, device_bank, rows):
        """bool[rows, input_dim]: the rows of a device bank, after a synchronisation."""
        self.sync()
        out = np.empty((int(rows), self.words), dtype=np.uint32)
        self._hip_check(self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(device_bank), out.nbytes, L.HIP_MEMCPY_DEVICE_TO_HOST),
                        "hipMemcpy")
        return np.unpackbits(out.view(np.uint8), axis=1, bitorder="little")[:, :self.input_dim].astype(np.bool_)

    # The record buffers are device memory of the HIP runtime the library itself is linked against (_lib.HIP_EXPORTS), kept for
    # the next recorded call and grown geometrically.
    def _record_buffer(self, field, elements):
        """Device address of a buffer of at least `elements` 32-bit words for one record field."""
        return self.kept_buffer(self._record_bufs, field, elements, spare=2)

    def _record_read(self, field, elements, dtype):
        """The first `elements` words of a record buffer (after sync())."""
        return self.read_words(self._record_bufs[field][0], elements, dtype)

    def device_buffer(self, nbytes, data=None, at_least=0):
        """Device address of `nbytes` new bytes (never fewer than `at_least`) on the engine's device (the caller frees them:
        hipFree), with the bytes of the numpy array `data` copied in."""
        ptr = C.c_void_p()
        self._hip_check(self.lib.hipSetDevice(self.device), "hipSetDevice")
        self._hip_check(self.lib.hipMalloc(C.byref(ptr), max(nbytes, at_least)), f"hipMalloc({nbytes} bytes)")
        if data is not None:
            self._hip_check(self.lib.hipMemcpy(ptr, data.ctypes.data_as(C.c_void_p), data.nbytes, L.HIP_MEMCPY_HOST_TO_DEVICE), "hipMemcpy")
        return ptr.value

    def kept_buffer(self, bufs, key, words, spare=1):
        """Device address of the buffer bufs[key] = (address, 32-bit words), kept across calls: made, or made anew when it holds
        fewer than `words` words -- then `spare` times its old size at least -- after waiting for the engine's stream (everything
        that used the old buffer is behind that) and freeing the old one."""
        ptr, size = bufs.get(key, (None, 0))
        if ptr is None or size < words:
            size = max(words, spare * size)
            new = self.device_buffer(4 * size)
            if ptr is not None:
                self.sync()
                self.lib.hipFree(ptr)
            ptr = new
            bufs[key] = (ptr, size)
        return ptr

    def read_words(self, device_words, elements, dtype):
        """The first `elements` 32-bit words at a device address (after sync())."""
        out = np.empty(elements, dtype=dtype)
        if elements:
            self._hip_check(self.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), device_words, 4 * elements, L.HIP_MEMCPY_DEVICE_TO_HOST),
                            "hipMemcpy")
        return out

    def _hip_check(self, rc, what):
        if rc != 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.hipGetErrorString(rc).decode()}")

    def graph_count(self):
        """hipGraphs this engine holds (htm_graph_count: captured and instantiated so far)."""
        return self._check(self.lib.htm_graph_count(self.h), "htm_graph_count")

    def prepare(self, device_bank, n_inputs, n_steps, learning=True, use_graph=True, pipeline=True, continuing=False, record=False,
                resets=None):
        """Build (capture + instantiate) the hipGraphs the run() call with these arguments will replay (`record`: a recorded
        run(), whatever its fields -- htm_prepare_recorded; `resets`: a run with reset bits, whichever)."""
        prepare, what = (self.lib.htm_prepare_recorded, "htm_prepare_recorded") if record else (self.lib.htm_prepare, "htm_prepare")
        with self.this_call(resets, n_inputs):
            self._check(prepare(self.h, C.c_void_p(device_bank), int(n_inputs), int(n_steps), int(bool(learning)),
                                run_flags(use_graph, pipeline, continuing)), what)

    def run_plan(self, n_steps, use_graph=True, pipeline=True, continuing=False, **_):
        """What a run() with these arguments would do now (htm_run_plan): dict(hip_graph, pipelined, lean, scan_large)."""
        bits = self._check(self.lib.htm_run_plan(self.h, int(n_steps), run_flags(use_graph, pipeline, continuing)), "htm_run_plan")
        return dict(hip_graph=bool(bits & L.PLAN_GRAPH), pipelined=bool(bits & L.PLAN_PIPELINED), lean=bool(bits & L.PLAN_LEAN),
                    scan_large=bool(bits & L.PLAN_SCAN_LARGE))

    # ---- column-sharded stepping (shard_world > 1): begin -> all-gather by the caller -> finish
    def shard_record_bytes(self):
        return int(self._check(self.lib.htm_shard_record_bytes(self.h), "htm_shard_record_bytes"))

    def shard_begin(self, send_ptr, input_bits=None, device_bank=None, n_inputs=1, learning=True):
        if input_bits is not None:
            packed = pack_bits(input_bits, self.words)
            rc = self.lib.htm_shard_begin(self.h, None, 1, packed.ctypes.data_as(C.c_void_p), int(bool(learning)), C.c_void_p(send_ptr))
        else:
            rc = self.lib.htm_shard_begin(self.h, C.c_void_p(device_bank), int(n_inputs), None, int(bool(learning)), C.c_void_p(send_ptr))
        self._check(rc, "htm_shard_begin")

    def shard_finish(self, recv_ptr, learning=True):
        self._check(self.lib.htm_shard_finish(self.h, C.c_void_p(recv_ptr), int(bool(learning))), "htm_shard_finish")
        self.steps += 1

    def shard_unique_id(self):
        """128-byte id for shard_comm_init (rank 0 creates it, the caller hands it to the other ranks)."""
        buf = C.create_string_buffer(128)
        rc = self.lib.htm_shard_unique_id(buf)
        if rc < 0:
            raise HtmError(f"htm_shard_unique_id failed ({rc}): {self.lib.htm_last_error(None).decode()}")
        return buf.raw

    def shard_comm_init(self, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.lib.htm_shard_comm_init(self.h, buf), "htm_shard_comm_init")

    def shard_comm_size(self):
        return int(self._check(self.lib.htm_shard_comm_size(self.h), "htm_shard_comm_size"))

    def shard_graph_ok(self):
        """Whether shard_run replays whole timesteps, the all-gather included, as hipGraphs (htm_shard_comm_init's preflight)."""
        return bool(self._check(self.lib.htm_shard_graph_ok(self.h), "htm_shard_graph_ok"))

    def shard_step(self, input_bits=None, device_bank=None, n_inputs=1, learning=True):
        """One column-sharded timestep with the exchange (RCCL) inside the library."""
        if input_bits is not None:
            packed = pack_bits(input_bits, self.words)
            rc = self.lib.htm_shard_step(self.h, None, 1, packed.ctypes.data_as(C.c_void_p), int(bool(learning)))
        else:
            rc = self.lib.htm_shard_step(self.h, C.c_void_p(device_bank), int(n_inputs), None, int(bool(learning)))
        self._check(rc, "htm_shard_step")
        self.steps += 1

    def populate(self, segments_per_cell, synapses=32, perm_lo=0.3, perm_hi=0.7, seed=0, cell_begin=0, cell_end=None):
        """Pre-populated pool generated on the device (htm_populate; BASELINE.json configs[4])."""
        if cell_end is None:
            cell_end = self.column_dim * self.cell_dim
        self._check(self.lib.htm_populate(self.h, int(cell_begin), int(cell_end), int(segments_per_cell), int(synapses),
                                          float(perm_lo), float(perm_hi), int(seed) & 0xFFFFFFFF), "htm_populate")

    def profile(self, enable):
        self._check(self.lib.htm_profile(self.h, int(bool(enable))), "htm_profile")

    def profile_read(self, max_kernels=64):
        names = (C.c_char_p * max_kernels)()
        ms = (C.c_double * max_kernels)()
        cnt = (C.c_int64 * max_kernels)()
        n = self._check(self.lib.htm_profile_read(self.h, max_kernels, names, ms, cnt), "htm_profile_read")
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def trace_read(self):
        """Device-clock timeline of the pipelined launches (handle created under BITHTM_TRACE=1):
        int64 array [slot = launch + 4 * step parity][block][start, end], 100 MHz ticks, 0 = not run."""
        buf = np.zeros(8 * 4096 * 2, np.uint64)
        self._check(self.lib.htm_trace_read(self.h, buf.ctypes.data_as(C.c_void_p), buf.size), "htm_trace_read")
        return buf.astype(np.int64).reshape(8, 4096, 2)

    # ---- State fields (host views of the last completed step)
    def read_sp_fields(self):
        return dict(
            active_column=self.read(L.F_ACTIVE_COLUMN, np.int32, self.active_columns).astype(np.int64),
            overlaps=self.read(L.F_OVERLAPS, np.int32, self.column_dim).astype(np.int64),
            boosted_overlaps=self.read(L.F_BOOSTED, np.float64, self.column_dim))

    def read_store(self):
        """The segment store.  On a column-sharded handle the per-segment arrays have one row per LOCAL row (the
        segments of the rank's own cells); `seg_gid` gives each row's global id (-1 = free row)."""
        info = self.info()
        S, E = info.local_segments, self.segment_slots
        return dict(
            S=info.segments, rows=S, slots=E, seg_gid=self.read(L.F_SEG_GID, np.int32, S),
            seg_cell=self.read(L.F_SEG_CELL, np.int32, S), seg_nsyn=self.read(L.F_SEG_NSYN, np.int32, S),
            presyn=self.read(L.F_SEG_PRESYN, np.int32, S * E).reshape(S, E),
            perm=self.read(L.F_SEG_PERM, np.float32, S * E).reshape(S, E),
            segcount=self.read(L.F_SEGCOUNT, np.int32, self.column_dim * self.cell_dim))

    def read_recyclable_counts(self):
        """The allocation's counts of recyclable segments (rows with fewer synapses than segment_matching_threshold) after the
        last completed step: (int32[nb] per 1 024 ids, int32[nb2] per 2^20 ids), nb = ceil(S / 1024), nb2 = ceil(nb / 1024)
        (HTM_F_RECYCLABLE_COUNTS; read only, not on a column-sharded handle).  They equal a recount from read_store()'s
        seg_nsyn: a test that reads them after every step sees a stale count before a later allocation acts on it."""
        nb = (self.info().segments + 1023) // 1024
        nb2 = (nb + 1023) // 1024
        out = self.read(L.F_RECYCLABLE_COUNTS, np.int32, nb + nb2)
        return out[:nb], out[nb:]

    def read_distal(self):
        """PredictiveProjection.State (projections.py:195-203) of the last step, segment ids
        ascending as np.where (projections.py:247) yields them."""
        info = self.info()
        if not info.has_distal_state:
            return None
        S, M, N = info.local_segments, info.matching_segments, self.column_dim * self.cell_dim
        seg = self.read(L.F_MATCH_SEGMENT, np.int32, M).astype(np.int64)
        minfo = self.read(L.F_MATCH_INFO, np.uint32, M)
        jit = self.read(L.F_MATCH_JITTER, np.float32, M)
        order = np.argsort(seg, kind="stable")
        seg, minfo, jit = seg[order], minfo[order], jit[order]
        active = (minfo >> 31).astype(np.bool_)
        seg_cell = self.read(L.F_SEG_CELL, np.int32, S)
        prediction = np.bincount(seg_cell[seg], weights=active, minlength=N).astype(np.float64)
        return dict(
            prediction=prediction,
            segment_potential=self.read(L.F_SEG_POTENTIAL, np.int32, S).astype(np.int64),
            matching_segment=seg, matching_segment_activation=((minfo >> 12) & 0xFFF).astype(np.int64),
            matching_segment_active=active, max_jittered_potential=self.read(L.F_CELL_MAX_JITTER, np.float32, N),
            matching_segment_jittered_potential=jit)

    # ---- state hand-off in the oracle's dictionary layout (oracle/htm_oracle.py export_state)
    def export_tm_state(self):
        info = self.check_capacity()
        K = self.cell_dim
        st = self.read_store()
        out = dict(
            S=np.int64(st["S"]), slots=np.int64(st["slots"]), step_index=np.int64(info.step_index),
            seg_cell=st["seg_cell"], seg_nsyn=st["seg_nsyn"], presyn=st["presyn"], perm=st["perm"], segcount=st["segcount"],
            prev_prediction=words_to_bool(self.read(L.F_CELL_PREDICTION, np.uint32, self.cell_words), K),
            prev_activation=words_to_bool(self.read(L.F_CELL_ACTIVATION, np.uint32, self.cell_words), K),
            prev_winner=self.read(L.F_WINNER_CELL, np.int32, info.winner_cells).astype(np.int64),
            has_prev_winner=np.bool_(info.has_winner_cells), has_distal=np.bool_(info.has_distal_state))
        if self.shard_world > 1:                    # rows are local: distributed.merge_shard_states puts the ranks' parts together
            out.update(seg_gid=st["seg_gid"], column_range=np.asarray(self.column_range))
        d = self.read_distal()
        if d is not None:
            out.update(d)
        return out

    def import_tm_state(self, st):
        K, S, E = self.cell_dim, int(st["S"]), self.segment_slots
        if "seg_gid" in st:
            raise HtmError("import_tm_state: this is one rank's part of a sharded state; merge the parts first (distributed.merge_shard_states)")
        if S > self.segment_capacity:
            raise CapacityError(f"state has {S} segments, pool holds {self.segment_capacity}")
        self._check(self.lib.htm_import_begin(self.h, int(st["step_index"])), "htm_import_begin")
        presyn = np.asarray(st["presyn"], dtype=np.int32).reshape(S, -1) if S else np.zeros((0, E), np.int32)      # (an empty store: a checkpoint of step 0)
        perm = np.asarray(st["perm"], dtype=np.float32).reshape(S, -1) if S else np.zeros((0, E), np.float32)
        nsyn = (presyn >= 0).sum(axis=1).astype(np.int32)
        if nsyn.max(initial=0) > E:
            raise CapacityError(f"a segment has {nsyn.max()} synapses, segment_slots is {E}")
        # rows are packed on the device: valid synapses first
        order = np.argsort(presyn < 0, axis=1, kind="stable")[:, :E] if presyn.shape[1] else np.zeros((S, 0), np.int64)
        p_presyn = np.full((S, E), -1, dtype=np.int32)
        p_perm = np.full((S, E), -1.0, dtype=np.float32)
        w = min(E, presyn.shape[1])
        p_presyn[:, :w] = np.take_along_axis(presyn, order, axis=1)[:, :w]
        p_perm[:, :w] = np.take_along_axis(perm, order, axis=1)[:, :w]
        self.write(L.F_SEG_CELL, st["seg_cell"], np.int32)
        self.write(L.F_SEG_NSYN, nsyn, np.int32)
        self.write(L.F_SEG_PRESYN, p_presyn, np.int32)
        self.write(L.F_SEG_PERM, p_perm, np.float32)
        self.write(L.F_SEGCOUNT, st["segcount"], np.int32)
        self.write(L.F_CELL_PREDICTION, bool_to_words(np.asarray(st["prev_prediction"]).reshape(self.column_dim, K)), np.uint32)
        self.write(L.F_CELL_ACTIVATION, bool_to_words(np.asarray(st["prev_activation"]).reshape(self.column_dim, K)), np.uint32)
        winners = np.asarray(st["prev_winner"], dtype=np.int32)
        self.write(L.F_WINNER_CELL, winners, np.int32)
        M = 0
        has_distal = bool(st["has_distal"])
        if has_distal:
            seg = np.asarray(st["matching_segment"], dtype=np.int32)
            M = len(seg)
            pot = np.asarray(st["segment_potential"], dtype=np.int64)
            minfo = (pot[seg].astype(np.uint32) | (np.asarray(st["matching_segment_activation"]).astype(np.uint32) << 12)
                     | (np.asarray(st["matching_segment_active"]).astype(np.uint32) << 31))
            self.write(L.F_SEG_POTENTIAL, pot, np.int32)
            self.write(L.F_MATCH_SEGMENT, seg, np.int32)
            self.write(L.F_MATCH_INFO, minfo, np.uint32)
            self.write(L.F_MATCH_JITTER, st["matching_segment_jittered_potential"], np.float32)
            self.write(L.F_CELL_MAX_JITTER, np.asarray(st["max_jittered_potential"], dtype=np.float32).view(np.uint32), np.uint32)
        self._check(self.lib.htm_import_commit(self.h, S, M, len(winners), int(has_distal), int(bool(st["has_prev_winner"]))),
                    "htm_import_commit")
        self.steps = int(st["step_index"])
