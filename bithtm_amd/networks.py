"""Drop-in counterparts of bithtm/networks.py: SpatialPooler, TemporalMemory,
HierarchicalTemporalMemory with the reference's constructor arguments, `process(...)`
(plus the alias `compute`), `State` records and `last_state`.

All computation happens in the HIP engine (bithtm_amd/csrc/htm_engine.hip) behind the C ABI;
this module is host logic: parameter plumbing, lazy read-back of State fields, and the
NumPy dtypes / shapes the reference returns.

Differences from the reference, all documented in DESIGN.md:
  * `active_column` comes back in ascending order (reference: np.argpartition order) and ties at
    the k-th boosted overlap go to the lower column index;
  * random tie-breaks use keyed draws (`seed=`), not the global np.random stream;
  * plug-in arguments (`proximal_projection=`, `boosting=`, `inhibition=`: networks.py:16,22-24) accept the objects
    of bithtm_amd.projections / bithtm_amd.regularizations (same constructor signatures as the reference's) -- the
    timestep is then one fused device call -- and ANY other object with the reference's `process` / `update`
    methods: SpatialPooler.process then runs phase by phase (htm_sp_phase), the device doing the parts that are
    its own and the user's object being called on the host for the others, exactly in the order of networks.py:26-35.
    `distal_projection=` (networks.py:50,55) likewise: a bithtm_amd PredictiveProjection is the device's segment store and the
    timestep stays fused; any other object with the reference's PredictiveProjection interface is called on the host from a
    host-side TemporalMemory.process (networks.py:91-128, `_process_host`).  `spatial_pooler=` / `temporal_memory=`
    (networks.py:134,143-144; example.py:7-12 swaps the Temporal Memory) take any object with `process`.
"""

import copy
import math
import weakref

import numpy as np

from . import _lib as L
from ._keyed import STREAM_INPUT_NOISE, draw_unit
from .likelihood import log_likelihood
from .engine import RECORD_COUNTERS, RECORD_FIELDS, SP_RECORD_FIELDS, SP_RECORD_TYPES, Engine, HtmError, check_lists, words_to_bool
from .projections import DenseProjection, PredictiveProjection
from .regularizations import ExponentialBoosting, GlobalInhibition, _Placeholder, checked_boosted, checked_overlaps


class _Lazy:
    """State base: fields are fetched from the device on first access while the engine still
    holds that step; the engine materialises every live State before it overwrites the step."""

    _fields = ()

    def __init__(self, engine, step):
        self._engine = engine
        self._step = step
        self._cache = {}
        engine._live_states.append(weakref.ref(self))

    @classmethod
    def _eager(cls, **fields):
        """A State that never was on a device: its fields are these values."""
        st = cls.__new__(cls)
        st._engine, st._step, st._cache = None, -1, fields
        return st

    def _fetch(self):
        raise NotImplementedError

    def _materialize(self):
        if self._engine is not None:
            if self._engine.steps != self._step:
                raise RuntimeError("State outlived its timestep without being materialised")
            self._cache.update(self._fetch())
            self._engine = None

    def __getattr__(self, name):
        if name.startswith("_") or name not in type(self)._fields:
            raise AttributeError(name)
        if name not in self._cache:
            self._materialize()
        return self._cache[name]

    def __setattr__(self, name, value):
        if name.startswith("_"):
            object.__setattr__(self, name, value)
        else:
            self._cache[name] = value


def retire_states(engine):
    """Called before a new step is enqueued: pin down every State somebody still holds (engine._live_states: weak references
    to the States of the current step -- a plain list: a host-fed step creates two and retires two, and this is on its path)."""
    live = engine._live_states
    if live:
        for ref in live:
            st = ref()
            if st is not None:
                st._materialize()
        live.clear()


class SpatialPooler:
    class State(_Lazy):
        """networks.py:8-12."""
        _fields = ("active_column", "overlaps", "boosted_overlaps")

        def _fetch(self):
            return self._engine.read_sp_fields()

    def __init__(self, input_dim, column_dim, active_columns, proximal_projection=None, boosting=None,
                 inhibition=None, device=0):
        self.input_dim = input_dim
        self.column_dim = column_dim
        self.active_columns = active_columns
        self.device = device
        self.proximal_projection = proximal_projection or DenseProjection(input_dim, column_dim)       # networks.py:22
        self.boosting = boosting or ExponentialBoosting(column_dim, active_columns)                    # :23
        self.inhibition = inhibition or GlobalInhibition(active_columns)                               # :24
        for name, obj, methods in (("proximal_projection", self.proximal_projection, ("process", "update")),
                                   ("boosting", self.boosting, ("process", "update")), ("inhibition", self.inhibition, ("process",))):
            if not all(callable(getattr(obj, m, None)) for m in methods):
                raise TypeError(f"{name} must have the reference's {' / '.join(methods)} methods; got {type(obj).__name__}")
        # which parts are the device's own (exact types: a subclass may override the methods the device would skip)
        self._own_proximal = type(self.proximal_projection) is DenseProjection
        self._own_boosting = type(self.boosting) is ExponentialBoosting
        self._own_inhibition = type(self.inhibition) is GlobalInhibition
        self._engine = None
        self._fused = False

    @property
    def _plain(self):
        return self._own_proximal and self._own_boosting and self._own_inhibition

    def _engine_parts(self):
        """The parameter objects the engine is built from: the user's where they are the device's own kind."""
        proximal = self.proximal_projection if self._own_proximal else _Placeholder(self.input_dim, self.column_dim)
        boosting = self.boosting if self._own_boosting else ExponentialBoosting(self.column_dim, self.active_columns)
        return proximal, boosting

    def _bind(self, engine, fused):
        self._engine, self._fused = engine, fused
        if self._own_proximal:
            self.proximal_projection._engine = engine
            self.proximal_projection._permanence = None      # now lives in device memory
        if self._own_boosting:
            self.boosting._engine = engine

    def _ensure_engine(self):
        if self._engine is None:
            proximal, boosting = self._engine_parts()
            self._bind(Engine(self.input_dim, self.column_dim, 0, self.active_columns, proximal=proximal, boosting=boosting,
                              device=self.device), False)
        return self._engine

    def _process_phases(self, input, learning, commit):
        """networks.py:26-35 with some of the three objects living on the host: the device runs the phases that are its
        own (htm_sp_phase), the user's objects are called for the others, in the reference's order."""
        eng = self._engine
        C = self.column_dim
        input = np.asarray(input, dtype=np.bool_)
        overlaps = boosted = None
        if self._own_proximal:
            eng.sp_phase(L.SP_OVERLAP, input)                                         # :27 (and :28 with the device's boosting)
        else:
            overlaps = np.asarray(self.proximal_projection.process(input))
            if self._own_boosting:                                                    # :28 (whole numbers, or a ValueError: never truncated)
                counts = checked_overlaps(overlaps, f"{type(self.proximal_projection).__name__}.process")
                eng.sp_phase(L.SP_BOOST, counts, np.int32)
        if not self._own_boosting:
            if overlaps is None:
                overlaps = eng.read(L.F_OVERLAPS, np.int32, C).astype(np.int64)
            boosted = np.asarray(self.boosting.process(overlaps))                     # :28
        if self._own_inhibition:
            # (a foreign boosting's values: finite and >= 0, or a ValueError; the State hands back the caller's own array)
            values = None if self._own_boosting else checked_boosted(boosted, f"{type(self.boosting).__name__}.process")
            eng.sp_phase(L.SP_SELECT, values, np.float64)                             # :29
            active_column = eng.read(L.F_ACTIVE_COLUMN, np.int32, self.active_columns).astype(np.int64)
        else:
            if boosted is None:
                boosted = eng.read(L.F_BOOSTED, np.float64, C)
            active_column = np.asarray(self.inhibition.process(boosted))              # :29
            eng.sp_phase(L.SP_ACTIVE, active_column, np.int32)
        if learning:                                                                  # :31-32
            if self._own_proximal:
                eng.sp_phase(L.SP_LEARN)
            else:
                self.proximal_projection.update(input, active_column)
        if self._own_boosting:                                                        # :33
            eng.sp_phase(L.SP_DUTY)
        else:
            self.boosting.update(active_column)
        if overlaps is None:
            overlaps = eng.read(L.F_OVERLAPS, np.int32, C).astype(np.int64)
        if boosted is None:
            boosted = eng.read(L.F_BOOSTED, np.float64, C)
        if commit:
            eng.sp_phase(L.SP_COMMIT)
        return self.State._eager(active_column=active_column, overlaps=overlaps, boosted_overlaps=boosted)

    def process(self, input, learning=True):
        """networks.py:26-35."""
        eng = self._ensure_engine()
        if self._fused:
            raise RuntimeError("this SpatialPooler is fused into a HierarchicalTemporalMemory; call its process()")
        retire_states(eng)
        if not self._plain:
            return self._process_phases(input, learning, commit=True)
        eng.sp_step(input, learning=learning)
        return self.State(eng, eng.steps)

    compute = process

    # run(noise=): steps per fill of the noise ring (as HierarchicalTemporalMemory.noise_chunk)
    noise_chunk = 1024

    def run(self, inputs, steps, learning=True, use_graph=True, record=None, noise=0.0, noise_seed=None, classifier=None, knn=None):
        """`steps` timesteps over the rows of the boolean matrix `inputs`, cycled: `steps` times
        process(inputs[t % n] ^ flip_noise(noise_seed, t, input_dim, noise), learning), t being this object's step index, with the
        bank resident in device memory and no per-step host work (htm_sp_run).  Everything the call leaves -- permanences, duty
        cycle, the State of the next process() -- is what that loop leaves, bit for bit, and successive calls compose: a and then b
        steps are one call of a + b.  The bank is uploaded once and kept until the inputs change.
        `record`: None (the call returns None), True (= ("active_column",)) or a tuple of "active_column", "active_overlap",
        "active_boosted": the call then returns an SPRunRecord over its `steps` steps, written on the device and read back once
        per call; `record.active_column` is what TemporalMemory.run takes as its lists.
        `noise`, `noise_seed`: as HierarchicalTemporalMemory.run's (drawn on the device into a ring the run reads instead of the
        bank, noise_chunk steps per fill; `noise_seed` defaults to 0); 0 is the run without noise, launch for launch.
        ValueError, before anything is created or enqueued: steps < 0, inputs that are not [n >= 1, input_dim], an unknown record
        name, noise outside [0, 1], a run that would pass step 2^32, a Spatial Pooler inside a fused HierarchicalTemporalMemory
        (call its run()), plug-in proximal_projection / boosting / inhibition objects (they step on the host: call process())."""
        _no_classifier(classifier, "SpatialPooler.run()")
        _no_knn(knn, "SpatialPooler.run()")
        if self._fused:
            raise ValueError("this SpatialPooler is fused into a HierarchicalTemporalMemory; call its run()")
        if not self._plain:
            raise ValueError("run() keeps the whole loop on the device: not available with plug-in proximal_projection / boosting / "
                             "inhibition objects; call process()")
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"steps must not be negative, got {steps}")
        inputs = np.asarray(inputs)
        if inputs.ndim != 2 or inputs.shape[0] < 1 or inputs.shape[1] != self.input_dim:
            raise ValueError(f"inputs: a boolean matrix [n >= 1, input_dim = {self.input_dim}], got shape {inputs.shape}")
        inputs = inputs.astype(np.bool_, copy=False)
        fields = None if record is None else _sp_record_fields(record)
        threshold = _noise_threshold_arg(noise)
        first = 0 if self._engine is None else self._engine.steps
        if first + steps > 1 << 32:
            raise ValueError("run(): the run would pass step 2^32, where the device's step counter wraps")
        eng = self._ensure_engine()
        retire_states(eng)
        n = inputs.shape[0]
        bank = _cached_bank(self, eng, inputs)
        noise_seed = (eng.seed if noise_seed is None else int(noise_seed)) if threshold else None
        parts = []
        for _, batch in _batches(steps, cap=int(self.noise_chunk) if threshold else None):
            if threshold:
                ring, _, rows = _noise_ring(self, eng, self.noise_chunk)
                eng.bank_noise(bank, n, ring, rows, eng.steps, batch, noise_seed, threshold)
                part = eng.sp_run(ring, rows, batch, learning=learning, use_graph=use_graph, record=fields)
            else:
                part = eng.sp_run(bank, n, batch, learning=learning, use_graph=use_graph, record=fields)
            parts.append(part)
        if fields is None:
            return None
        k = self.active_columns
        whole = {f: parts[0][f] if len(parts) == 1 else np.concatenate([p[f] for p in parts]) if parts else np.zeros((0, k), SP_RECORD_TYPES[f][0])
                 for f in fields}
        return SPRunRecord(first + np.arange(steps, dtype=np.int64), **whole)


class SPRunRecord:
    """What SpatialPooler.run(record=...) returns: one numpy array per field over the steps of the call, step i of the call in row
    i, the k = active_columns winners of a step in ascending column order (include/bithtm_hip.h, htm_sp_run).
      step_index       int64[steps]        timesteps processed before each step (the engine's step index)
      active_column    int32[steps, k]     sp_state.active_column of each step ("active_column", else None)
      active_overlap   int32[steps, k]     sp_state.overlaps[active_column] ("active_overlap", else None)
      active_boosted   float64[steps, k]   sp_state.boosted_overlaps[active_column] ("active_boosted", else None)
      fields           the names recorded, in this order"""

    def __init__(self, step_index, active_column=None, active_overlap=None, active_boosted=None):
        self.step_index = np.asarray(step_index, dtype=np.int64)
        self.active_column, self.active_overlap, self.active_boosted = active_column, active_overlap, active_boosted
        self.fields = tuple(f for f in SP_RECORD_FIELDS if getattr(self, f) is not None)

    def __len__(self):
        return len(self.step_index)


def _sp_record_fields(record):
    """SpatialPooler.run(record=...) -> the fields asked for, each once, in SP_RECORD_FIELDS order: True = the winner lists; else
    a name or a tuple of names."""
    if record is True:
        return ("active_column",)
    fields = (record,) if isinstance(record, str) else tuple(record)
    if not fields or set(fields) - set(SP_RECORD_FIELDS):
        raise ValueError(f"record: True or a tuple of {SP_RECORD_FIELDS} (got {record!r})")
    return tuple(f for f in SP_RECORD_FIELDS if f in fields)


class TemporalMemory:
    class State(_Lazy):
        """networks.py:39-46; `distal_state` mirrors PredictiveProjection.State (projections.py:195-203)."""
        _fields = ("active_cell", "winner_cell", "cell_activation", "cell_prediction", "active_column_bursting",
                   "distal_state")

        def __init__(self, engine, step, active_column=None):
            self._active_column = active_column
            super().__init__(engine, step)

        def _fetch(self):
            eng = self._engine
            C, K = eng.column_dim, eng.cell_dim
            info = eng.check_capacity()          # an overflowed pool must not be read as if nothing happened
            cols = self._active_column
            if cols is None:
                cols = eng.read(L.F_ACTIVE_COLUMN, np.int32, eng.active_columns).astype(np.int64)
            cols = np.asarray(cols, dtype=np.int64)             # in the CALLER's order, as the reference indexes with it
            act = words_to_bool(eng.read(L.F_CELL_ACTIVATION, np.uint32, eng.cell_words), K)
            rows, cells = np.where(act[cols])                                        # networks.py:116-117
            bursting = np.empty(len(cols), dtype=np.bool_)      # (the device keeps it by ascending column)
            bursting[np.argsort(cols, kind="stable")] = eng.read(L.F_BURSTING, np.uint8, eng.active_columns)[:len(cols)].astype(np.bool_)
            out = dict(
                cell_activation=act,
                cell_prediction=words_to_bool(eng.read(L.F_CELL_PREDICTION, np.uint32, eng.cell_words), K),
                active_cell=(cols[rows], cells),
                active_column_bursting=bursting[:, None],
                winner_cell=None)
            if info.has_winner_cells:
                winner = words_to_bool(eng.read(L.F_WINNER_WORDS, np.uint32, eng.cell_words), K)
                rows, cells = np.where(winner[cols])                                 # networks.py:103-104
                out["winner_cell"] = (cols[rows], cells)
            d = eng.read_distal()
            out["distal_state"] = None if d is None else _DistalState(d)
            return out

    def __init__(self, column_dim, cell_dim, distal_projection=None, seed=0, device=0):
        self.column_dim = column_dim
        self.cell_dim = cell_dim
        self.seed = seed
        self.device = device
        self.distal_projection = distal_projection or PredictiveProjection(self.column_dim * self.cell_dim)     # networks.py:55
        # the device's own kind (exact type: a subclass may override the methods the fused step would skip) -- or any object
        # with the reference's PredictiveProjection interface, which is then called on the host (_process_host)
        # (more than 64 cells per column: the device's Temporal Memory step is built on one or two 32-bit words of cells per
        # column -- a lane per cell, a half-wave or a wave per column; the segment store is not -- it lives in cell space -- so
        # such a model keeps its projection on the device and runs the per-column part of TemporalMemory.process,
        # networks.py:95-119, on the host: correct, not fast)
        self._own_distal = type(self.distal_projection) is PredictiveProjection and cell_dim <= 64
        if not self._own_distal:
            if isinstance(self.distal_projection, PredictiveProjection):      # a subclass of the device's: tell it the model's shape
                self.distal_projection.cell_dim, self.distal_projection.seed = cell_dim, seed
            missing = [m for m in ("process", "update", "get_jittered_potential_info") if not callable(getattr(self.distal_projection, m, None))]
            missing += [a for a in ("segment_matching_threshold", "bundle_segments") if a not in dir(self.distal_projection)]
            if missing:
                raise TypeError(f"distal_projection must have the reference's PredictiveProjection interface; "
                                f"{type(self.distal_projection).__name__} lacks {', '.join(missing)}")
        self._host_step = 0
        self._host_last = None
        self._engine = None
        self._fused = False
        self._last_ref = None             # weak: an unread State costs nothing
        self._last_cols = None
        self._empty_state = self.get_empty_state()                                   # networks.py:57
        self._was_reset = False           # reset() since the last step: last_state is the empty state

    def _bind(self, engine, fused):
        self._engine, self._fused = engine, fused
        self.distal_projection._engine = engine

    def _ensure_engine(self, n_active):
        if self._engine is None:
            self._bind(Engine(0, self.column_dim, self.cell_dim, n_active, distal=self.distal_projection,
                              seed=self.seed, device=self.device), False)
        return self._engine

    def grow_pool(self, segment_capacity=None, segment_slots=None):
        """The reference's segment store grows on demand (DynamicArray2D.add_rows / add_cols, utils.py:113-135); the
        device's pool has a fixed capacity.  This re-creates the engine with a larger pool (default: twice the segments)
        and hands the state over -- a host round trip.  Pools left at their default size grow by themselves (see
        Engine.pool_look); an explicit `segment_capacity=` is a hard limit and overflowing it raises CapacityError."""
        if self._fused:
            raise RuntimeError("this TemporalMemory is fused into a HierarchicalTemporalMemory; call its grow_pool()")
        eng = self._ensure_engine(1)
        retire_states(eng)
        dp = self.distal_projection
        dp.segment_capacity = int(segment_capacity or 2 * eng.segment_capacity)
        dp.segment_slots = int(segment_slots or eng.segment_slots)
        self._recreate(eng, eng.active_columns).carry_from(eng)
        self._last_ref = None

    def _recreate(self, eng, n_active):
        """A new engine for n_active active columns and the distal projection's pool sizes, with the state of `eng`."""
        bigger = Engine(0, self.column_dim, self.cell_dim, n_active, distal=self.distal_projection, seed=self.seed, device=self.device)
        if eng.steps:
            bigger.import_tm_state(eng.export_tm_state())
        self._bind(bigger, False)
        return bigger

    def get_empty_state(self):
        """networks.py:59-65."""
        return TemporalMemory.State._eager(
            active_cell=(np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32)), winner_cell=None,
            cell_activation=np.zeros((self.column_dim, self.cell_dim), dtype=np.bool_),
            cell_prediction=np.zeros((self.column_dim, self.cell_dim), dtype=np.bool_),
            active_column_bursting=np.empty(0, dtype=np.bool_), distal_state=None)

    def flatten_cell(self, cell):
        """networks.py:67-71."""
        if cell is None:
            return None
        assert len(cell) == 2 and len(cell[0].shape) == 1
        return cell[0] * self.cell_dim + cell[1]

    @property
    def last_state(self):
        """networks.py:57,127.  Held weakly: the State of the latest step is only read back from
        the device if somebody asks for it."""
        if not self._own_distal:
            return self._host_last if self._host_last is not None else self._empty_state
        if self._was_reset:
            return self._empty_state
        st = self._last_ref() if self._last_ref is not None else None
        if st is None:
            if self._engine is None or self._engine.steps == 0:
                return self._empty_state
            st = self._new_state(self._last_cols)
        return st

    @last_state.setter
    def last_state(self, state):
        """The reference's sequence reset, `tm.last_state = tm.get_empty_state()` (networks.py:57-65,91-93): assigning an
        empty State (no predicted cell, distal_state None) is reset(); assigning the current last_state changes nothing.
        Any other State cannot be adopted here -- process(prev_state=...) takes it for one step."""
        if state is self.last_state:
            return
        if _is_empty_state(state):
            self.reset()
            return
        raise ValueError("last_state only takes get_empty_state() (a sequence reset) or itself; "
                         "pass any other State to process(prev_state=...)")

    def reset(self):
        """A sequence reset: the next step runs as after `last_state = get_empty_state()` -- no predictions (every active
        column bursts), no distal state (no learning of the distal segments in that step), no winner cells.  The segment
        store, the step index and epsilon stay.  On the device (htm_reset: one launch, no host copy, no wait); a model whose
        distal projection lives on the host only forgets its host-side last state."""
        if not self._own_distal:
            self._host_last = None
            return
        if self._engine is not None and self._engine.steps > 0:
            retire_states(self._engine)
            self._engine.reset()
        self._last_ref = None
        self._was_reset = True

    def _new_state(self, active_column=None):
        st = self.State(self._engine, self._engine.steps, active_column)
        self._last_ref, self._last_cols = weakref.ref(st), active_column
        self._was_reset = False
        return st

    def process(self, sp_state, prev_state=None, learning=True, return_winner_cell=True, epsilon=1e-8):
        """networks.py:91-128.  `prev_state`: None / this object's `last_state` (the previous step's state lives in
        device memory), or any State this object returned earlier -- its fields are then written back as the device's
        previous step (a host round trip).  `epsilon` (the tolerance of the best-matching / least-used ties, as
        float32): any value in (0, 1]."""
        if not self._own_distal:
            return self._process_host(sp_state, prev_state, learning, return_winner_cell, epsilon)
        adopt = None
        if prev_state is not None and prev_state is not self.last_state:
            if _is_empty_state(prev_state):                                 # a sequence reset: htm_reset, not the host import
                adopt = "reset"
            else:
                d = prev_state.distal_state                                 # (reading the fields materialises a lazy State)
                adopt = (prev_state.cell_prediction, prev_state.cell_activation,
                         None if prev_state.winner_cell is None else self.flatten_cell(prev_state.winner_cell), d)
        if not 0.0 < epsilon <= 1.0:
            raise NotImplementedError("epsilon must lie in (0, 1]")
        if self._fused:
            raise RuntimeError("this TemporalMemory is fused into a HierarchicalTemporalMemory; call its process()")
        active_column = np.asarray(sp_state.active_column, dtype=np.int64)
        eng = self._ensure_engine(max(len(active_column), 1))
        retire_states(eng)
        eng = self._engine_for(eng, len(active_column))
        eng.use_epsilon(epsilon)
        if eng.pool_look(max(len(active_column), 1)):
            self.grow_pool(*eng._grow_to)
            eng = self._engine
            eng.use_epsilon(epsilon)
        if adopt == "reset":
            eng.reset()
        elif adopt is not None:
            eng.import_prev_state(*adopt)
        eng.tm_step(active_column, learning=learning, return_winner_cell=return_winner_cell)
        return self._new_state(active_column)

    def _engine_for(self, eng, n_active):
        """The reference takes any number of active columns: where `eng` holds fewer, a larger engine with the same state (and
        a pool of the size the distal projection names: one that has grown since is a fixed size from here on)."""
        if n_active <= eng.active_columns:
            return eng
        return self._recreate(eng, max(n_active, 2 * eng.active_columns))

    def run(self, active_columns, steps, learning=True, use_graph=True, record=None, resets=None, classifier=None, knn=None):
        """`steps` timesteps over the rows of `active_columns` (int [n_rows, n]: n distinct column ids per row, in any order),
        cycled: `steps` times process(SimpleNamespace(active_column=active_columns[t % n_rows]), learning=learning), t being this
        object's step index, with the lists resident in device memory and no per-step host work (htm_tm_run).  Everything the
        call leaves -- last_state, the segment store -- is what that loop leaves, bit for bit.  The lists are checked once per
        array (ValueError for an id outside [0, column_dim) or twice in a row) and kept on the device.
        `record`: as HierarchicalTemporalMemory.run's -- True for the counters, or a tuple of "counters", "active_column" (each
        step's sorted list, int32[steps, n]) and "column_prediction"; the call then returns a RunRecord.  "predicted_input" raises
        ValueError: a stand-alone Temporal Memory has no proximal mask to decode with.
        `resets`: a bool per row -- reset() before every step that reads a row whose flag is set, on the device inside the run.
        ValueError for cell_dim above 64 and for a plug-in distal_projection (both step on the host: call process()), and for a
        Temporal Memory inside a fused HierarchicalTemporalMemory (call its run())."""
        _no_classifier(classifier, "TemporalMemory.run()")
        _no_knn(knn, "TemporalMemory.run()")
        if self._fused:
            raise ValueError("this TemporalMemory is fused into a HierarchicalTemporalMemory; call its run()")
        if self.cell_dim > 64:
            raise ValueError("run(): cell_dim above 64 steps on the host; call process()")
        if not self._own_distal:
            raise ValueError("run() keeps the whole loop on the device: not available with a plug-in distal_projection; call process()")
        fields = None if record is None else _record_fields(record)
        if fields and {"predicted_input", "predicted_value"} & set(fields):
            raise ValueError("run(record='predicted_input'): a stand-alone TemporalMemory has no proximal mask to decode with")
        lists = check_lists(active_columns, self.column_dim)
        n_rows, n = lists.shape
        steps = int(steps)
        if steps < 0:
            raise ValueError(f"steps must not be negative, got {steps}")
        if resets is not None:
            resets = np.asarray(resets, dtype=np.bool_).ravel()
            if resets.shape != (n_rows,):
                raise ValueError(f"resets: one flag per row of active_columns ({n_rows}), got {resets.shape[0]}")
        eng = self._ensure_engine(n)
        retire_states(eng)
        eng = self._engine_for(eng, n)
        # A pool left at its default size grows as in HierarchicalTemporalMemory.run: batches the free segments are expected to
        # last (2 x n new segments per step), with a look at the pool between them
        call = _BatchedCall([self], fields)
        del eng                                     # (the pool step may re-create the engine: the old one goes, device memory and all, as it does)
        for _, batch in _batches(steps, lambda: [(_looked_at_pool(self, 2 * n), 2 * n, 1)]):
            eng = self._engine
            eng.use_epsilon(1e-8)                           # (process()'s default, which this loop is made of)
            part = eng.tm_run(eng.upload_lists(lists, check=False), n_rows, n, batch, learning=learning, use_graph=use_graph, record=fields,
                              resets=None if resets is None else eng.upload_resets(resets), check=False)
            if fields is not None and "active_column" in part:
                part["active_column"] = part["active_column"][:, :n]
            call.add([part])
        return call.finish([steps], [n], [lists[(self._engine.steps - 1) % n_rows].astype(np.int64)] if steps else [])[0]

    def _process_host(self, sp_state, prev_state, learning, return_winner_cell, epsilon):
        """networks.py:91-128 on the host, for a `distal_projection=` object that lives there: its `process` / `update` /
        `get_jittered_potential_info` are called exactly where the reference calls them.  The columns are processed in
        ascending order and the "least used" jitter is the keyed draw of the device (policies 1 and 3)."""
        from ._keyed import draw_unit, STREAM_LEAST_USED
        dp, C, K = self.distal_projection, self.column_dim, self.cell_dim
        eps = np.float32(epsilon)
        if prev_state is None:
            prev_state = self.last_state                                                          # :92-93
        caller_cols = np.asarray(sp_state.active_column, dtype=np.int64)
        order = np.argsort(caller_cols, kind="stable")
        active_column = caller_cols[order]
        pred = np.asarray(prev_state.cell_prediction)[active_column].reshape(len(active_column), K)    # :96
        bursting = ~pred.any(axis=1, keepdims=True)                                               # :97
        winner_cell = None
        if learning or return_winner_cell:
            if prev_state.distal_state is None:                                                   # :74-75
                column_matching = np.zeros((len(active_column), 1), dtype=np.bool_)
                best = np.zeros((len(active_column), K), dtype=np.bool_)
            else:                                                                                 # :76-82
                cell_max, _ = dp.get_jittered_potential_info(prev_state.distal_state)
                cell_max = np.asarray(cell_max, dtype=np.float32).reshape(C, K)[active_column]
                column_max = cell_max.max(axis=1, keepdims=True) if len(active_column) else cell_max[:, :1]
                column_matching = column_max >= dp.segment_matching_threshold
                best = np.abs(cell_max - column_max) < eps
            count = np.asarray(dp.bundle_segments).reshape(C, K)[active_column].astype(np.float32)    # :85-86
            flat = active_column[:, None] * K + np.arange(K)
            jit = (count.astype(np.float64) + draw_unit(self.seed, STREAM_LEAST_USED, self._host_step, flat)).astype(np.float32)   # :87
            least = np.abs(jit - jit.min(axis=1, keepdims=True)) < eps if len(active_column) else jit.astype(np.bool_)   # :88
            winner = pred | (bursting & np.where(column_matching, best, least))                   # :102
            rows, cells = np.where(winner)                                                        # :103-104
            winner_cell = (active_column[rows], cells)
        if learning:                                                                              # :106-113
            column_punishment = np.ones(C, dtype=np.bool_)
            column_punishment[active_column] = False
            dp.update(prev_state.distal_state, np.asarray(prev_state.cell_activation).reshape(-1), self.flatten_cell(winner_cell),
                      np.repeat(column_punishment, K), winner_input=self.flatten_cell(prev_state.winner_cell), epsilon=epsilon)
        activated = pred | bursting                                                               # :115
        rows, cells = np.where(activated)
        active_cell = (active_column[rows], cells)
        cell_activation = np.zeros((C, K), dtype=np.bool_)
        cell_activation[active_column] = activated                                                # :118-119
        distal_state = dp.process(self.flatten_cell(active_cell), return_jittered_potential_info=return_winner_cell)   # :121
        cell_prediction = np.asarray(distal_state.prediction).reshape(C, K) > epsilon             # :122
        caller_bursting = np.empty_like(bursting)
        caller_bursting[order] = bursting                                                         # (per column, in the caller's order)
        st = TemporalMemory.State._eager(active_cell=active_cell, winner_cell=winner_cell, cell_activation=cell_activation,
                                         cell_prediction=cell_prediction, active_column_bursting=caller_bursting,
                                         distal_state=distal_state)
        self._host_last = st
        self._host_step += 1
        return st

    compute = process


def _is_empty_state(state):
    """get_empty_state() as the step after it sees it: no predicted cell and no distal state (networks.py:59-65)."""
    return state.distal_state is None and not np.any(np.asarray(state.cell_prediction))


class _DistalState:
    """PredictiveProjection.State (projections.py:195-203)."""

    def __init__(self, d):
        self.__dict__.update(d)


class RunRecord:
    """What HierarchicalTemporalMemory.run(record=...) returns: one numpy array per field over the steps of the call, step i
    of the call in row i (include/bithtm_hip.h, htm_run_recorded, for the meaning of every count).
      step_index                     int64[steps]   timesteps processed before each step (the engine's step index)
      active_columns, bursting_columns, predicted_columns_before, predicted_columns, active_cells, winner_cells, segments,
      new_segments                   int32[steps]   the counters ("counters"; None when not recorded)
      active_column                  int32[steps, k]   sp_state.active_column of each step ("active_column", else None)
      column_prediction              bool[steps, C]    cell_prediction.any(axis=1) of each step ("column_prediction", else None)
      predicted_input                int32[steps, input_dim]   the predicted-input votes of the state each step leaves
                                                       (HierarchicalTemporalMemory.predicted_input; "predicted_input", else None)
      predicted_bucket, predicted_score   int32[steps, F]   those votes decoded per field of the run's encoder, on the device
                                                       (ScalarEncoder.decode; "predicted_value", else None)
      predicted_value                float64[steps, F] encoder.value_of(predicted_bucket): NaN where nothing is predicted
      anomaly_likelihood             float64[steps]    with run(likelihood=): the anomaly likelihood of each step (likelihood.py), else
                                                       None; log_likelihood is NuPIC's log scale of it
      classified_bucket              int32[steps, H]   with run(classifier=): per horizon of the SDRClassifier the most probable bucket
                                                       (classifier.py), classified_probability float64[steps, H] its probability (p /
                                                       65536) and, for a classifier of an encoder field, classified_value float64
                                                       [steps, H] = field.value_of(bucket); else None
      class_distribution             int32[steps, H, buckets]   all probabilities in units of 2^-16 ("class_distribution", else None)
      knn_label, knn_votes, knn_overlap, knn_nearest_slot, knn_nearest_step   int32[steps]   with run(knn=): the label most of the
                                                       KNNClassifier's nearest stored patterns carry (-1: no neighbour) and its votes,
                                                       the nearest one's overlap, slot and storing step (knn.py); else None
      knn_votes_all                  int32[steps, labels]   every label's votes ("knn_votes_all", else None)
    and, from the counters, the per-step report of example.py:55-57 and the raw anomaly score:
      correct_columns   = active_columns - bursting_columns
      incorrect_columns = predicted_columns_before - correct_columns
      anomaly_score     = 1 - correct_columns / active_columns   (float64; 0 for a step without active columns)"""

    def __init__(self, step_index, counters=None, active_column=None, column_prediction=None, predicted_input=None,
                 predicted_bucket=None, predicted_score=None, predicted_value=None, anomaly_likelihood=None, classified=None,
                 class_distribution=None, classified_field=None, knn=None, knn_votes_all=None):
        self.step_index = np.asarray(step_index, dtype=np.int64)
        self.fields = tuple(f for f, v in zip(RECORD_FIELDS, (counters, active_column, column_prediction, predicted_input, predicted_bucket))
                            if v is not None)
        for i, name in enumerate(RECORD_COUNTERS):
            setattr(self, name, None if counters is None else np.ascontiguousarray(counters[:, i], dtype=np.int32))
        self.active_column = active_column
        self.column_prediction = column_prediction
        self.predicted_input = predicted_input
        self.predicted_bucket, self.predicted_score, self.predicted_value = predicted_bucket, predicted_score, predicted_value
        self.anomaly_likelihood = anomaly_likelihood
        self.classified_bucket = self.classified_probability = self.classified_value = None
        if classified is not None:              # int32 [steps, H, 2]: (bucket, p in units of 2^-16)
            self.classified_bucket = np.ascontiguousarray(classified[:, :, 0])
            self.classified_probability = classified[:, :, 1].astype(np.float64) / 65536.0
            if classified_field is not None:
                self.classified_value = classified_field.value_of(self.classified_bucket)
        self.class_distribution = class_distribution
        for i, name in enumerate(KNN_ROW):      # int32 [steps, 5]: knn.ROW order
            setattr(self, name, None if knn is None else np.ascontiguousarray(knn[:, i]))
        self.knn_votes_all = knn_votes_all

    def __len__(self):
        return len(self.step_index)

    @property
    def correct_columns(self):
        return None if self.active_columns is None else self.active_columns - self.bursting_columns

    @property
    def incorrect_columns(self):
        return None if self.active_columns is None else self.predicted_columns_before - self.correct_columns

    @property
    def anomaly_score(self):
        if self.active_columns is None:
            return None
        active = self.active_columns.astype(np.float64)
        return np.where(active > 0, 1.0 - self.correct_columns / np.maximum(active, 1.0), 0.0)

    @property
    def log_likelihood(self):
        return None if self.anomaly_likelihood is None else log_likelihood(self.anomaly_likelihood)


KNN_ROW = ("knn_label", "knn_votes", "knn_overlap", "knn_nearest_slot", "knn_nearest_step")


def _record_fields(record):
    """run(record=...) -> the fields asked for: True = the counters; else a tuple of RECORD_FIELDS names."""
    if record is True:
        return ("counters",)
    fields = (record,) if isinstance(record, str) else tuple(record)
    if not fields or set(fields) - set(RECORD_FIELDS):
        raise ValueError(f"record: True or a tuple of {RECORD_FIELDS} (got {record!r})")
    return tuple(f for f in RECORD_FIELDS if f in fields)


class HierarchicalTemporalMemory:
    """networks.py:131-149.  With default (or bithtm_amd) components both layers share ONE device
    engine and a timestep is a single C-ABI call (`htm_step`)."""

    def __init__(self, input_dim, column_dim, cell_dim, active_columns=None, spatial_pooler=None,
                 temporal_memory=None, seed=0, device=0, stream=None):
        """`stream`: None (the engine creates a stream of its own), or the address of a hipStream_t to enqueue on, given as an
        object with a `handle` attribute that must outlive the engine (model groups: ModelGroup.create puts its members on one)."""
        if active_columns is None:
            active_columns = round(column_dim * 0.02)                                # networks.py:137
        self.column_dim = column_dim
        self.cell_dim = cell_dim
        self.active_columns = active_columns
        self.spatial_pooler = spatial_pooler or SpatialPooler(input_dim, column_dim, active_columns, device=device)    # :143
        self.temporal_memory = temporal_memory or TemporalMemory(column_dim, cell_dim, seed=seed, device=device)       # :144
        sp, tm = self.spatial_pooler, self.temporal_memory
        for name, obj in (("spatial_pooler", sp), ("temporal_memory", tm)):
            if not callable(getattr(obj, "process", None)):
                raise TypeError(f"{name} must have the reference's process method; got {type(obj).__name__}")
        # Both layers the device's own: ONE engine, one C call per timestep.  Any other object (example.py:7-12 swaps the
        # Temporal Memory this way) -- or a Temporal Memory whose distal projection lives on the host -- is called as
        # networks.py:146-149 calls it, each device-backed layer then stepping an engine of its own.
        self._engine = None
        if type(sp) is SpatialPooler and type(tm) is TemporalMemory and tm._own_distal:
            if sp._engine is not None or tm._engine is not None:
                raise ValueError("spatial_pooler / temporal_memory must not have been stepped on their own before fusing")
            proximal, boosting = sp._engine_parts()
            self._engine = Engine(sp.input_dim, column_dim, cell_dim, sp.active_columns,
                                  proximal=proximal, boosting=boosting, distal=tm.distal_projection,
                                  seed=tm.seed, device=device, stream=None if stream is None else stream.handle, stream_owner=stream)
            sp._bind(self._engine, True)
            tm._bind(self._engine, True)

    @property
    def engine(self):
        return self._engine

    def grow_pool(self, segment_capacity=None, segment_slots=None):
        """A larger segment pool (default: twice the segments) under the same model: the engine is re-created and the
        whole state handed over (see TemporalMemory.grow_pool; utils.py:113-135 is what the reference does instead)."""
        eng = self._fused_engine("grow_pool()")
        state = self.state_dict()
        sp, tm = self.spatial_pooler, self.temporal_memory
        dp = tm.distal_projection
        dp.segment_capacity = int(segment_capacity or 2 * eng.segment_capacity)
        dp.segment_slots = int(segment_slots or eng.segment_slots)
        proximal, boosting = sp._engine_parts()
        if sp._own_proximal:
            proximal._engine, proximal._permanence = None, state["sp_permanence"]      # (the new engine uploads it)
        owner = eng._stream_owner                   # (the stream the model was created on, if it was given one)
        bigger = Engine(sp.input_dim, self.column_dim, self.cell_dim, sp.active_columns, proximal=proximal, boosting=boosting,
                        distal=dp, seed=tm.seed, device=tm.device, stream=None if owner is None else owner.handle, stream_owner=owner)
        bigger.carry_from(eng)
        self._engine = bigger
        sp._bind(bigger, True)
        tm._bind(bigger, True)
        self.load_state_dict(state)
        self._bank = None

    def process(self, input, learning=True):
        """networks.py:146-149."""
        eng = self._engine
        if eng is None:                             # a layer that is not the device's own: the reference's two calls
            sp_state = self.spatial_pooler.process(input, learning=learning)
            return sp_state, self.temporal_memory.process(sp_state, learning=learning)
        retire_states(eng)
        if eng.pool_look(self.active_columns):
            self.grow_pool(*eng._grow_to)
            eng = self._engine
        if not self.spatial_pooler._plain:          # plug-in objects on the host: SP phase by phase, then the TM with its winners
            sp_state = self.spatial_pooler._process_phases(input, learning, commit=False)
            eng.tm_step(sp_state.active_column, learning=learning)
            return sp_state, self.temporal_memory._new_state(sp_state.active_column)
        eng.step(input, learning=learning)
        sp_state = SpatialPooler.State(eng, eng.steps)
        tm_state = self.temporal_memory._new_state(None)
        return sp_state, tm_state

    compute = process

    def reset(self):
        """A sequence reset before the next step: `temporal_memory.last_state = temporal_memory.get_empty_state()`, the
        reference's idiom (networks.py:57-65,91-93), which this also accepts.  See TemporalMemory.reset."""
        reset = getattr(self.temporal_memory, "reset", None)
        if callable(reset):
            reset()
        else:                                       # a plug-in Temporal Memory with the reference's interface only
            self.temporal_memory.last_state = self.temporal_memory.get_empty_state()

    # ---- checkpoint / resume (the reference has none).  The dictionary holds the
    # reference's own arrays: DenseProjection.permanence, ExponentialBoosting.duty_cycle, and the
    # SparseProjection / PredictiveProjection store + last State in the layout of oracle export_state.
    def _fused_engine(self, what):
        if self._engine is None:
            raise RuntimeError(f"{what} needs both layers on the device (one engine); this model has a layer or a distal projection that lives on the host")
        return self._engine

    def state_dict(self):
        eng = self._fused_engine("state_dict()")
        retire_states(eng)
        out = {"tm_" + k: np.asarray(v) for k, v in eng.export_tm_state().items()}
        out["sp_permanence"] = eng.get_permanence()
        out["sp_duty_cycle"] = eng.read_duty_cycle()
        return out

    def load_state_dict(self, state):
        eng = self._fused_engine("load_state_dict()")
        retire_states(eng)
        eng.set_permanence(np.asarray(state["sp_permanence"], dtype=np.float64))
        eng.write(L.F_DUTY_CYCLE, np.asarray(state["sp_duty_cycle"], dtype=np.float32), np.float32)
        eng.import_tm_state({k[3:]: v for k, v in state.items() if k.startswith("tm_")})
        self.temporal_memory._last_ref = None
        self.temporal_memory._was_reset = False

    def save(self, path):
        np.savez_compressed(path, **self.state_dict())

    def load(self, path):
        with np.load(path) as z:
            self.load_state_dict({k: z[k] for k in z.files})

    def _run_args(self, eng, what, inputs, steps, record, resets, noise, noise_seed, encoder=None):
        """The arguments of a batched call over `inputs` (run(), lookahead()), checked -> (noise threshold or 0, record fields
        or None, noise seed, inputs as a bool matrix -- with an `encoder`, as the float64 matrix of its values -- resets as a bool
        vector or None)."""
        threshold = _noise_threshold_arg(noise)
        fields = None if record is None else _record_fields(record)
        _check_encoder(encoder, fields, eng.input_dim, self.column_dim)
        if threshold:
            if eng.shard_world > 1:
                raise ValueError(f"{what}(noise=): not available on a column-sharded model")
            if eng.steps + max(steps, 0) + 1 > 1 << 32:
                raise ValueError(f"{what}(noise=): the run would pass step 2^32, where the device's step counter wraps")
            noise_seed = eng.seed if noise_seed is None else int(noise_seed)
        inputs = np.asarray(inputs, dtype=np.bool_) if encoder is None else encoder.bank_values(inputs)
        if resets is not None:
            resets = np.asarray(resets, dtype=np.bool_).ravel()
            if resets.shape != (inputs.shape[0],):
                raise ValueError(f"resets: one flag per row of inputs ({inputs.shape[0]}), got {resets.shape[0]}")
        return threshold, fields, noise_seed, inputs, resets

    def _batch_source(self, eng, bank, inputs, resets, fill, threshold, noise_seed):
        """What one batch of a batched call reads -> (device bank, its rows, its reset bits or None): the bank of `inputs`, or
        with noise the ring, filled here (enqueued) with the rows of the `fill` steps from the engine's current one -- the
        batch's and the one behind it -- and with the ring's reset bits where the caller gave flags."""
        if not threshold:
            return bank, inputs.shape[0], None if resets is None else eng.upload_resets(resets)
        ring, ring_resets, rows = _noise_ring(self, eng, self.noise_chunk)
        flags = eng.upload_resets(resets if resets is not None else np.zeros(inputs.shape[0], dtype=np.bool_))
        eng.bank_noise(bank, inputs.shape[0], ring, rows, eng.steps, fill, noise_seed, threshold, flags, ring_resets)
        return ring, rows, None if resets is None else ring_resets

    def run(self, inputs, steps, learning=True, use_graph=True, pipeline=True, continuing=False, record=None, resets=None,
            noise=0.0, noise_seed=None, encoder=None, likelihood=None, classifier=None, targets=None, classifier_learning=None,
            knn=None, labels=None, knn_learning=None):
        """`steps` timesteps over the rows of the boolean matrix `inputs`, cycled, with the input
        bank resident in device memory and no per-step host work (the loop of example.py:48-53).
        Returns None; read `temporal_memory.last_state` or call process() afterwards.  `continuing=True`: the
        caller streams its input in chunks and the next call is another run() on the same inputs (HTM_RUN_CONTINUE:
        the Spatial Pooler keeps working ahead across the calls; finish with a run() without it).
        `record`: a per-step record written on the device and read back once per call (htm_run_recorded) -- True for the
        counters, or a tuple of "counters", "active_column", "column_prediction", "predicted_input"; the call then returns a
        RunRecord over its `steps` steps.
        `resets`: a bool per row of `inputs` -- a sequence reset (see reset()) before every step that reads a row whose flag is
        set, on the device inside the run; the flags are uploaded beside the bank and kept with it.
        `noise`: p in [0, 1] -- every step reads its row with fresh flip noise, process(inputs[t % n] ^ flip_noise(noise_seed, t,
        input_dim, p)) with t this model's step index (the stream of example.py:52 under the keyed generator; `noise_seed`
        defaults to the model's seed).  The noise is drawn on the device (htm_bank_noise) into a ring of noise_chunk + 2 rows
        that the run reads instead of the bank, noise_chunk steps per fill; it depends on (seed, step, input) alone, so calls of
        a and b steps draw what one call of a + b steps draws, and it never repeats with the bank.  0 (the default) is the run
        without noise, launch for launch.  `resets` keeps its meaning (a flag per row of `inputs`, expanded on the device).
        `encoder`: a ScalarEncoder whose input_dim is the model's -- `inputs` is then float64 [n, F], the VALUES of its F fields:
        run(values, steps, encoder=enc) is run(enc.encode(values), steps), bit for bit, with the values uploaded once (8 F bytes
        per row) and the bank encoded on the device (htm_bank_encode) and kept until the values change; everything else --
        resets, noise, streaming, records -- works over that bank unchanged.  With it `record` may name "predicted_value": each
        step's votes decoded on the device per field (htm_decode_votes, one launch per batch behind the run; steps x F x 2 ints
        read back, the votes themselves only if "predicted_input" is asked for too) into RunRecord.predicted_bucket, _score,
        _value.  None (the default) is the call as it was, launch for launch.
        `likelihood`: an AnomalyLikelihood of one stream -- the run records its counters (as record=True; named fields are
        recorded too), behind each batch the likelihood's update is enqueued over the batch's record buffer before the read-back
        (htm_likelihood_update: the run still waits once per batch), and RunRecord.anomaly_likelihood holds each step's value.
        The object's state continues across calls; the model's resets do not touch it.
        `classifier`: an SDRClassifier -- the run records its counters, every step leaves its active-cell words on the device
        (htm_set_run_active_cells: one small launch per step) and behind each batch the classifier's update over them is enqueued
        before the read-back (htm_classifier_update: the run still waits once per batch).  `targets`: int [rows of inputs], the
        bucket of each row (-1: missing; ValueError at or above the classifier's buckets), uploaded once; None with `encoder`: the
        bucket of classifier.field among the encoder's fields, taken with encoder.bucket on the host.  A step's target is its own
        row's; a reset flag of a row also empties the classifier's history.  `classifier_learning`: None follows `learning`.
        RunRecord.classified_bucket, _probability, _value hold each step's prediction per horizon, and with "class_distribution"
        named in `record`, RunRecord.class_distribution all probabilities.
        `knn`: a KNNClassifier -- it rides on the run as the classifier does, over the same captured active-cell words (one
        capture launch per step, shared when both are given), its update enqueued next to the classifier's behind each batch
        (htm_knn_update: a fixed number of launches per 64 steps).  `labels`: int [rows of inputs], the label of each row (-1, or
        anything outside [0, knn.labels): none), uploaded once; None: nothing is labelled.  A step's label is its own row's; a
        labelled step of a learning call is stored after it was inferred.  `knn_learning`: None follows `learning`.  ValueError
        before anything is enqueued when the call's labelled steps do not fit knn.capacity.  The model's resets do not touch the
        object.  RunRecord.knn_label, knn_votes, knn_overlap, knn_nearest_slot, knn_nearest_step hold each step's result, and with
        "knn_votes_all" named in `record`, RunRecord.knn_votes_all every label's votes."""
        if classifier is not None:
            from .sdr_classifier import SDRClassifierBank
            if isinstance(classifier, SDRClassifierBank):            # (many streams; this call has one)
                _no_classifier(classifier, "run() with an SDRClassifierBank")
        eng = self._fused_engine("run()")
        cls = None
        if classifier is not None:
            distribution = record is not None and record is not True and "class_distribution" in ((record,) if isinstance(record, str) else tuple(record))
            if distribution:
                record = tuple(f for f in ((record,) if isinstance(record, str) else tuple(record)) if f != "class_distribution") or None
            record = _with_counters(record)
            if eng.shard_world > 1:
                raise ValueError("run(classifier=): not available on a column-sharded model")
            cls = dict(clf=classifier, distribution=distribution, learn=bool(learning if classifier_learning is None else classifier_learning))
        elif targets is not None or classifier_learning is not None:
            raise ValueError("run(): targets= and classifier_learning= go with classifier=")
        near = None
        if knn is not None:
            from .knn_classifier import KNNClassifierBank
            if isinstance(knn, KNNClassifierBank):                  # (many streams; this call has one)
                _no_knn(knn, "run() with a KNNClassifierBank")
            named = () if record is None or record is True else ((record,) if isinstance(record, str) else tuple(record))
            if "knn_votes_all" in named:
                record = tuple(f for f in named if f != "knn_votes_all") or None
            record = _with_counters(record)
            if eng.shard_world > 1:
                raise ValueError("run(knn=): not available on a column-sharded model")
            near = dict(knn=knn, votes="knn_votes_all" in named, learn=bool(learning if knn_learning is None else knn_learning))
        elif labels is not None or knn_learning is not None:
            raise ValueError("run(): labels= and knn_learning= go with knn=")
        if likelihood is not None:
            if likelihood.streams != 1:
                raise ValueError(f"run(likelihood=): an AnomalyLikelihood of one stream, got {likelihood.streams}")
            record = _with_counters(record)
        if not self.spatial_pooler._plain:
            raise RuntimeError("run() keeps the whole loop on the device: not available with plug-in objects that live on the host")
        steps = int(steps)
        threshold, fields, noise_seed, inputs, resets = self._run_args(eng, "run", inputs, steps, record, resets, noise, noise_seed, encoder)
        retire_states(eng)
        if cls is not None:
            from .sdr_classifier import model_shape
            classifier._set_shape(*model_shape(eng))
            cls["host_targets"] = _classifier_targets(classifier, targets, inputs, encoder)
            cls["rows"] = inputs.shape[0]
        if near is not None:
            from .sdr_classifier import model_shape
            knn._set_shape(*model_shape(eng))
            near["host_labels"] = knn.check_labels(np.full(inputs.shape[0], -1) if labels is None else labels)
            if near["host_labels"].shape != (inputs.shape[0],):
                raise ValueError(f"labels: one label per row of inputs ({inputs.shape[0]}), got {near['host_labels'].shape[0]}")
            knn.check_room(knn.stored_by(near["host_labels"], eng.steps % inputs.shape[0], steps, near["learn"]))
        bank = _cached_bank(self, eng, inputs, encoder=encoder)
        # A pool left at its default size grows like the reference's arrays (utils.py:113-135): the run is cut into batches
        # the free segments are expected to last (2 x active_columns new segments per step: every column bursting, twice),
        # with a look at the pool between them.  An overflow inside a batch is still reported, never silent.
        k = self.active_columns
        call = _BatchedCall([self.temporal_memory], fields, encoder, likelihood is not None, classifier, knn)
        del eng                                     # (the pool step may re-create the engine: the old one goes, device memory and all, as it does)
        refuse = "the segment pool has to grow in the middle of a streamed run(): end the stream (a run() without continuing=True) first"

        def regrown():
            nonlocal bank
            bank = _cached_bank(self, self._engine, inputs, fresh=True, encoder=encoder)

        def pool():
            return [(_looked_at_pool(self, 2 * k, self._streaming and refuse, regrown), 2 * k, 1)]
        for done, n in _batches(steps, pool, cap=int(self.noise_chunk) if threshold else None):
            eng = self._engine
            last = done + n >= steps
            # (a streamed call ends with the Spatial Pooler ahead: it has read the row of the step behind the batch and, in the
            # four-launch schedule, of the one behind that -- one row more; the next call's fill writes those rows again with the
            # words they have)
            src, rows, bits = self._batch_source(eng, bank, inputs, resets, n + (2 if continuing and last else 1), threshold, noise_seed)
            if cls is not None:                     # (targets and reset bits by the row of `inputs` a step reads, whatever bank the run reads)
                if "targets" not in cls:
                    cls["targets"] = classifier.upload_targets(eng, cls["host_targets"])
                cls["resets"] = None if resets is None else eng.upload_resets(resets)
            if near is not None and near.get("engine") is not eng:      # (the labels by the row of `inputs` a step reads, as the targets)
                near["labels"], near["engine"] = knn.upload_labels(eng, near["host_labels"]), eng
            call.add([eng.run(src, rows, n, learning=learning, use_graph=use_graph, pipeline=pipeline, continuing=continuing and last,
                              record=fields, resets=bits, encoder=encoder, likelihood=likelihood, classifier=cls, knn=near)])
            self._streaming = bool(continuing and last and pipeline)
        return call.finish([steps], [k])[0]

    _streaming = False                              # in the middle of a streamed run(): the last one ended with continuing=True

    # run(noise=): steps per fill of the noise ring (the ring holds two rows more); an attribute so that a caller, or a test, can
    # cut a noisy run into smaller batches
    noise_chunk = 1024

    def inference_view(self):
        """An InferenceView of this model: a model that shares this one's weights -- the Spatial Pooler's permanences, the segment
        store -- in device memory and steps a stream of its own with learning=False (htm_create_view).  It starts as this model
        would be after reset(): same duty cycles and step index, no Temporal Memory state.  This model may keep learning; its
        views always step on its current weights.  Many views in a ModelGroup read the store once per step together."""
        eng = self._viewable_engine("inference_view()")
        retire_states(eng)
        return InferenceView(self)

    def _viewable_engine(self, what):
        """The engine of a model that views can be made of; ValueError (`what`: the caller's name) for any other."""
        eng = self._engine
        if eng is None or not self.spatial_pooler._plain:
            raise ValueError(f"{what} needs both layers on the device (one engine): this model has a layer, a distal "
                             "projection or plug-in objects that live on the host")
        if getattr(self.temporal_memory, "cell_dim", 0) > 64:
            raise ValueError(f"{what}: cell_dim above 64 steps on the host")
        if eng.shard_world > 1:
            raise ValueError(f"{what}: views of column-sharded models are not available")
        if self._streaming:
            raise ValueError(f"{what}: this model is in the middle of a streamed run() (continuing=True): end the stream first")
        return eng

    def fork(self):
        """A new InferenceView that CONTINUES this model's stream: inference_view(), then its stream state made this model's
        current one on the device (InferenceView.sync; htm_view_sync -- one launch, nothing goes through the host).  Stepping the
        fork equals stepping a full copy of this model (load_state_dict(state_dict()), no reset()) with learning=False, bit for
        bit; this model is not changed and may keep learning.  fork().forecast(k) is what this model expects over the next k
        steps from where it is now.  ValueError where inference_view() raises it, and for a model with a step open phase by
        phase (the library refuses to make the view)."""
        self._viewable_engine("fork()")
        try:
            view = self.inference_view()
        except HtmError as e:
            raise ValueError(f"fork(): {e}") from e
        return view.sync(self)

    # lookahead(): windows per chunk.  Inside a chunk nothing is waited for or read back; at its end the host waits once and
    # reads the chunk's forecast rows and records.  The chunk bounds the device buffers (chunk x horizon bank rows, chunk x every
    # record rows: at 256 windows of horizon 50 and input_dim 1024 the rows are 1.6 MB) and 256 windows are at least 512 steps of
    # device work, against which one wait (a few tens of microseconds) is noise; a larger chunk buys nothing measurable.  An
    # attribute so that a caller, or a test, can cut a look-ahead into smaller chunks.
    lookahead_chunk = 256

    def _forkable_engine(self, what):
        """The engine of a model fork() works on (a view overrides this: its parent is what views are made of)."""
        return self._viewable_engine(what)

    def _lookahead_fork(self):
        """The fork lookahead() forecasts on: one per engine, kept, made anew when the engine was re-created."""
        kept = getattr(self, "_la_fork", None)
        if kept is None or kept[0]() is not self._engine:
            fork = self.fork()                      # (ValueError for a model that has no engine to fork)
            self._la_fork = kept = (weakref.ref(self._engine), fork)
        return kept[1]

    def lookahead(self, inputs, steps, horizon, min_votes=1, max_bits=0, every=1, learning=True, use_graph=True, record=None,
                  resets=None, noise=0.0, noise_seed=None, encoder=None, classifier=None, knn=None):
        """Rolling look-ahead: the model runs over `inputs` as run() does (learning or not) and after every `every` steps says
        what it expects over the next `horizon` steps, its own stream unmoved.  Bit for bit, with W = steps // every:
            for j in range(W):
                run(inputs, every, learning=, record=, resets=, noise=, noise_seed=)
                rows[j] = fork().forecast(horizon, min_votes, max_bits)
        Returns rows, bool[W, horizon, input_dim], or with `record` the pair (rows, RunRecord over the `steps` steps); the model
        is left exactly where run(inputs, steps, ...) leaves it.  On the device, per window: the model's steps, one launch that
        makes a kept fork's stream state the model's (htm_view_sync), the fork's feedback run of `horizon` steps, and a copy of
        its rows into a result buffer -- nothing waited for or read back inside a chunk of `lookahead_chunk` windows; a
        default-sized pool is looked at between chunks, as in run().  ValueError: steps not a multiple of every, horizon < 1,
        every < 1, and what fork(), run() and forecast() refuse.  `encoder`: as run()'s -- `inputs` are then values, and the
        record may name "predicted_value" (decoded once per chunk behind its windows)."""
        _no_classifier(classifier, "lookahead()")
        _no_knn(knn, "lookahead()")
        steps, horizon, every = int(steps), int(horizon), int(every)
        if horizon < 1 or every < 1:
            raise ValueError(f"lookahead(): horizon and every must be at least 1, got {horizon} and {every}")
        if steps < 0 or steps % every:
            raise ValueError(f"lookahead(): steps ({steps}) must be a multiple of every ({every})")
        min_votes, max_bits = _encode_params(min_votes, max_bits)
        eng = self._forkable_engine("lookahead()")
        threshold, fields, noise_seed, inputs, resets = self._run_args(eng, "lookahead", inputs, steps, record, resets, noise, noise_seed, encoder)
        if encoder is None and (inputs.ndim != 2 or inputs.shape[0] < 1 or inputs.shape[1] != eng.input_dim):
            raise ValueError(f"inputs: bool [n_inputs, {eng.input_dim}], got {inputs.shape}")
        self._lookahead_fork()                      # (behind every check of the arguments: a refused call makes no view)
        retire_states(eng)
        bank = _cached_bank(self, eng, inputs, encoder=encoder)
        k, bank_rows = self.active_columns, horizon + 1
        rows = np.zeros((steps // every, horizon, eng.input_dim), dtype=np.bool_)
        call = _BatchedCall([self.temporal_memory], fields, encoder)
        del eng                                     # (as in run(): the pool step may re-create the engine)

        def regrown():
            nonlocal bank
            bank = _cached_bank(self, self._engine, inputs, fresh=True, encoder=encoder)

        def pool():
            return [(_looked_at_pool(self, 2 * k, None, regrown), 2 * k, 1)]
        for done, n in _batches(steps, pool, cap=max(int(self.lookahead_chunk), 1) * every, multiple=every):
            eng, fork = self._engine, self._lookahead_fork()
            feng, windows = fork._engine, n // every
            shapes = eng.record_shapes(encoder)
            record_bufs = {} if fields is None else eng._record_buffers(fields, n, encoder)
            fbank = fork._zero_bank(feng, bank_rows)
            out = feng.kept_buffer(feng._record_bufs, "lookahead_rows", windows * horizon * feng.words)
            with feng.this_call(feedback=(fbank, bank_rows, min_votes, max_bits)):
                for j in range(windows):
                    for at, m in _batches(every, cap=int(self.noise_chunk) if threshold else None):
                        src, src_rows, bits = self._batch_source(eng, bank, inputs, resets, m + 1, threshold, noise_seed)
                        with eng.this_call(bits, src_rows):
                            eng.run_into(src, src_rows, m, {f: ptr + 4 * (j * every + at) * shapes[f][0] for f, ptr in record_bufs.items()},
                                         learning=learning, use_graph=use_graph)
                    feng.view_sync(eng)
                    first = feng.steps
                    feng.encode_votes(min_votes, max_bits, fbank, bank_rows, first % bank_rows)
                    feng.run_into(fbank, bank_rows, horizon, {}, learning=False, use_graph=use_graph)
                    feng.bank_rows(fbank, bank_rows, first, horizon, out + 4 * j * horizon * feng.words)
            eng.decode_records(record_bufs, n, encoder)
            call.add([None if fields is None else eng._records_read(fields, n, sync=True, encoder=encoder)])
            feng.sync()
            words = feng.read_words(out, windows * horizon * feng.words, np.uint32).reshape(windows, horizon, feng.words)
            rows[done // every:done // every + windows] = np.unpackbits(words.view(np.uint8), axis=2, bitorder="little")[:, :, :feng.input_dim]
            self._streaming = False
        record = call.finish([steps], [k])[0]
        return rows if fields is None else (rows, record)

    def predicted_input(self):
        """Which input the model expects next: int32[input_dim], the votes of the predicted columns for the inputs they are
        connected to -- for the state the last step left, (pp.permanence[tm_state.cell_prediction.any(axis=1)] >=
        pp.permanence_threshold).sum(axis=0) with pp = spatial_pooler.proximal_projection (include/bithtm_hip.h,
        htm_predicted_input).  One launch and one read-back of input_dim words."""
        eng = self._engine
        if eng is None:
            raise RuntimeError("predicted_input() decodes on the device: not available with a layer or a distal projection that lives on the host")
        if not self.spatial_pooler._plain:
            raise RuntimeError("predicted_input() decodes on the device: not available with plug-in Spatial Pooler objects that live on the host")
        return eng.predicted_input()

    def predicted_value(self, encoder):
        """Which VALUE the model expects next, per field of `encoder`: (value float64[F], score int32[F]) = the votes of
        predicted_input() decoded on the device (htm_predicted_value: the votes launch, the decode launch and a read-back of
        2 F ints; the votes never reach the host) -- encoder.decode(predicted_input()), the value encoder.value_of of the
        bucket.  A fresh or reset model gives NaN and 0."""
        if self._engine is None or not self.spatial_pooler._plain:
            raise RuntimeError("predicted_value() decodes on the device: not available with layers or plug-in objects that live on the host")
        encoder.check_model(self._engine.input_dim, self.column_dim)
        bucket, score = self._engine.predicted_value(encoder)
        return encoder.value_of(bucket), score

    def forecast_values(self, steps, encoder, min_votes=1, max_bits=0, use_graph=True):
        """The values the model expects at horizons 1 .. steps: (value float64[steps, F], score int32[steps, F]).  The loop is
        forecast(steps, min_votes, max_bits) and the state left is its state; row j is the decode of the votes that forecast
        row x_j encodes -- row 0 from the state before the call (predicted_value's path), row j >= 1 from the state forecast
        step j - 1 leaves (the recorded rows, decoded on the device).  No votes cross to the host."""
        steps = int(steps)
        eng = self._forecast_engine("forecast_values()")
        encoder.check_model(eng.input_dim, self.column_dim)
        bucket = np.full((max(steps, 0), len(encoder)), -1, dtype=np.int32)
        score = np.zeros_like(bucket)
        if steps > 0:
            bucket[0], score[0] = eng.predicted_value(encoder)
            _, rec = self.forecast(steps, min_votes, max_bits, record=("predicted_value",), use_graph=use_graph, encoder=encoder)
            bucket[1:], score[1:] = rec.predicted_bucket[:-1], rec.predicted_score[:-1]
        return encoder.value_of(bucket), score

    # forecast(): steps per feeding run (the device bank holds one row more); an attribute so that a caller, or a test, can cut a
    # forecast into smaller runs
    forecast_chunk = 1024

    def _forecast_engine(self, what):
        eng = self._fused_engine(what)
        if not self.spatial_pooler._plain:
            raise RuntimeError(f"{what} keeps the whole loop on the device: not available with plug-in objects that live on the host")
        if self._streaming:
            raise RuntimeError(f"{what} in the middle of a streamed run() (continuing=True): end the stream first")
        return eng

    def _zero_bank(self, eng, rows):
        """A device bank of `rows` rows on `eng` for forecast() / predicted_bits(), kept (so that the graphs of feeding runs, which
        are keyed by the bank, are reused across calls) until the engine is re-created."""
        banks = getattr(self, "_forecast_banks", None)
        if banks is None or banks[0]() is not eng:
            self._forecast_banks = banks = (weakref.ref(eng), {})
        if rows not in banks[1]:
            banks[1][rows] = eng.zero_bank(rows)
        return banks[1][rows]

    def predicted_bits(self, min_votes=1, max_bits=0):
        """bool[input_dim]: the input the model expects next, as forecast() would feed it back -- encode_votes(predicted_input(),
        min_votes, max_bits), encoded on the device (htm_encode_votes): one launch sequence and one read-back of a packed row."""
        min_votes, max_bits = _encode_params(min_votes, max_bits)
        eng = self._forecast_engine("predicted_bits()")
        retire_states(eng)
        bank = self._zero_bank(eng, 1)
        eng.encode_votes(min_votes, max_bits, bank, 1, 0)
        return eng.read_bank(bank, 1)[0]

    def forecast(self, steps, min_votes=1, max_bits=0, record=None, use_graph=True, learning=False, noise=0.0, encoder=None, classifier=None,
                 knn=None):
        """What the model expects over the next `steps` steps: from its current state, `steps` times
            x = encode_votes(predicted_input(), min_votes, max_bits);  process(x, learning=False)
        with the whole loop on the device (htm_set_run_feedback: each step's votes are encoded into the bank row the next step
        reads).  Returns the x of every step, bool[steps, input_dim]; with `record` (as run(record=)) the pair (rows, RunRecord).
        The state it leaves, and everything the record holds, are those of that loop bit for bit.  An input with fewer than
        min_votes votes is never set, so a row may be empty -- and stays empty once the model predicts nothing.  learning=True
        (learning from the model's own output) raises ValueError.  To look ahead without moving this model's own stream,
        forecast on a view:  view = htm.inference_view(); view.run(context, n); view.forecast(k).  `noise` other than 0 raises
        ValueError: a forecast reads the rows the model itself wrote, and flipping them is not offered.  `encoder`: the
        ScalarEncoder a "predicted_value" record decodes with (forecast_values() is the call that returns values)."""
        _no_classifier(classifier, "forecast()")
        _no_knn(knn, "forecast()")
        if learning:
            raise ValueError("forecast(): learning from the model's own output is not available (learning=False only)")
        if _noise_threshold_arg(noise):
            raise ValueError("forecast(): input noise inside a forecast is not available (run(noise=) flips the rows of a bank)")
        min_votes, max_bits = _encode_params(min_votes, max_bits)
        eng = self._forecast_engine("forecast()")
        fields = None if record is None else _record_fields(record)
        _check_encoder(encoder, fields, eng.input_dim, self.column_dim)
        retire_states(eng)
        chunk = int(self.forecast_chunk)
        bank = self._zero_bank(eng, chunk + 1)
        rows = np.zeros((int(steps), eng.input_dim), dtype=np.bool_)
        call = _BatchedCall([self.temporal_memory], fields, encoder)
        for done, n in _batches(steps, cap=chunk):          # (a forecast never looks at the pool: it does not learn)
            s0 = eng.steps
            eng.encode_votes(min_votes, max_bits, bank, chunk + 1, s0 % (chunk + 1))
            with eng.this_call(feedback=(bank, chunk + 1, min_votes, max_bits)):
                call.add([eng.run(bank, chunk + 1, n, learning=False, use_graph=use_graph, record=fields, encoder=encoder)])
            rows[done:done + n] = eng.read_bank(bank, chunk + 1)[(s0 + np.arange(n)) % (chunk + 1)]
        record = call.finish([int(steps)], [self.active_columns])
        return rows if fields is None else (rows, record[0])


def _check_encoder(encoder, fields, input_dim, column_dim):
    """The `encoder=` of a batched call: ValueError for one that does not fit the model, and for a "predicted_value" record
    without one."""
    if encoder is not None:
        encoder.check_model(input_dim, column_dim)
    elif fields and "predicted_value" in fields:
        raise ValueError('record "predicted_value" needs an encoder (encoder=): it says which bits are which field')


def _encode_params(min_votes, max_bits):
    min_votes, max_bits = int(min_votes), int(max_bits)
    if min_votes < 1 or max_bits < 0:
        raise ValueError(f"min_votes must be at least 1 and max_bits at least 0 (0 = no cap); got {min_votes}, {max_bits}")
    return min_votes, max_bits


def encode_votes(votes, min_votes=1, max_bits=0):
    """The input row forecast() feeds back for the votes of predicted_input(): bool[input_dim], votes >= min_votes, and with
    max_bits > 0 at most the max_bits inputs with the most votes (ties at the cut-off go to the lower input index).  The NumPy
    definition of what htm_encode_votes computes on the device."""
    min_votes, max_bits = _encode_params(min_votes, max_bits)
    votes = np.asarray(votes)
    x = votes >= min_votes
    if max_bits and x.sum() > max_bits:
        keep = np.lexsort((np.arange(votes.size), -votes.astype(np.int64)))[:max_bits]
        x = np.zeros(votes.size, dtype=np.bool_)
        x[keep] = True
    return x


def noise_threshold(p):
    """ceil(p * 2**24): the integer the device compares a 24-bit draw m with, m < noise_threshold(p) being m * 2**-24 < p for
    every integer m (p * 2**24 is exact in float64).  ValueError unless 0 <= p <= 1."""
    p = float(p)
    if not 0.0 <= p <= 1.0:                         # (a NaN fails both comparisons)
        raise ValueError(f"noise must lie in [0, 1], got {p}")
    return int(math.ceil(p * 16777216.0))


def _noise_threshold_arg(noise):
    """run(noise=) -> noise_threshold(noise); 0 = no noise.  One number: a per-member list belongs to ModelGroup.run."""
    if np.ndim(noise) != 0:
        raise ValueError(f"noise: one probability in [0, 1], got an array of shape {np.shape(noise)}")
    return noise_threshold(noise)


def flip_noise(seed, step, input_dim, p):
    """bool[input_dim]: the inputs run(noise=p, noise_seed=seed) flips in the step with index `step` -- example.py:52's
    np.random.rand(input_dim) < p with the keyed generator's stream 6 in place of np.random.rand:
    draw_unit(seed, STREAM_INPUT_NOISE, step mod 2**32, arange(input_dim)) < p.  The NumPy definition of what htm_bank_noise
    draws on the device."""
    noise_threshold(p)
    return draw_unit(seed, STREAM_INPUT_NOISE, int(step) & 0xFFFFFFFF, np.arange(int(input_dim), dtype=np.uint32)) < float(p)


class InferenceView(HierarchicalTemporalMemory):
    """A model that shares its parent's weights in device memory and owns only its stream state (HierarchicalTemporalMemory.
    inference_view(); include/bithtm_hip.h htm_create_view).  process() and run() default to learning=False, and learning=True
    raises ValueError; reset(), predicted_input(), last_state and the States work as on the parent.  state_dict(), save(),
    load_state_dict() and grow_pool() raise ValueError: save the parent.  A view is a member of a ModelGroup like any model.

    The parent may keep learning between view calls; a view always steps on the parent's current weights.  If the parent's
    engine is re-created (grow_pool(), by hand or by its growing default pool), the view raises ValueError: make new views."""

    def __init__(self, parent):
        eng = Engine.view_of(parent._engine)
        self.column_dim, self.cell_dim, self.active_columns = parent.column_dim, parent.cell_dim, parent.active_columns
        sp, tm = copy.copy(parent.spatial_pooler), copy.copy(parent.temporal_memory)
        # (the view's own copies of the parameter objects, bound to the view's engine: they read the shared weights through it,
        # and hold no reference to the parent's engine -- which goes when the parent does)
        sp.proximal_projection, sp.boosting = copy.copy(sp.proximal_projection), copy.copy(sp.boosting)
        tm.distal_projection = copy.copy(tm.distal_projection)
        sp._bind(eng, True)
        tm._bind(eng, True)
        tm._last_ref, tm._last_cols, tm._host_last = None, None, None
        tm._was_reset = True
        self.spatial_pooler, self.temporal_memory = sp, tm
        self._engine = eng
        self._parent = weakref.ref(parent)
        self._parent_engine = weakref.ref(parent._engine)

    def _check_parent(self):
        parent = self._parent()
        if parent is not None and parent._engine is not self._parent_engine():
            raise ValueError("the parent model's engine was re-created (grow_pool() or its pool's growth) since this view was "
                             "made: this view still holds the old weights; make a new view with parent.inference_view()")

    @staticmethod
    def _no_learning(learning, what):
        if learning:
            raise ValueError(f"{what}: an inference view steps with learning=False only (it shares its parent's weights)")

    def process(self, input, learning=False):
        self._no_learning(learning, "process()")
        self._check_parent()
        return super().process(input, learning=False)

    compute = process

    def run(self, inputs, steps, learning=False, use_graph=True, pipeline=True, continuing=False, record=None, resets=None,
            noise=0.0, noise_seed=None, encoder=None, likelihood=None, classifier=None, targets=None, classifier_learning=None,
            knn=None, labels=None):
        """As the parent's run(), with learning=False.  `classifier_learning` may be True: the classifier's weights are its own, not
        the parent's.  `knn`: a view never stores -- its steps are inferred over the store as it is (`labels` are taken and ignored)."""
        self._no_learning(learning, "run()")
        self._check_parent()
        return super().run(inputs, steps, learning=False, use_graph=use_graph, pipeline=pipeline, continuing=continuing,
                           record=record, resets=resets, noise=noise, noise_seed=noise_seed, encoder=encoder, likelihood=likelihood,
                           classifier=classifier, targets=targets, classifier_learning=classifier_learning, knn=knn, labels=labels,
                           knn_learning=None if knn is None else False)

    def reset(self):
        self._check_parent()
        super().reset()

    def predicted_input(self):
        self._check_parent()
        return super().predicted_input()

    def predicted_bits(self, min_votes=1, max_bits=0):
        self._check_parent()
        return super().predicted_bits(min_votes, max_bits)

    def forecast(self, steps, min_votes=1, max_bits=0, record=None, use_graph=True, learning=False, noise=0.0, encoder=None):
        self._check_parent()
        return super().forecast(steps, min_votes, max_bits, record=record, use_graph=use_graph, learning=learning, noise=noise,
                                encoder=encoder)

    def predicted_value(self, encoder):
        self._check_parent()
        return super().predicted_value(encoder)

    def forecast_values(self, steps, encoder, min_votes=1, max_bits=0, use_graph=True):
        self._check_parent()
        return super().forecast_values(steps, encoder, min_votes, max_bits, use_graph=use_graph)

    def sync(self, source=None):
        """This view's stream becomes that of `source` -- the parent (the default) or another view of the same parent -- as it is
        now, on the device (htm_view_sync: one launch, no host copy, no wait): from here the view steps as a full copy of the
        source would with learning=False, and last_state reads as the source's.  The source is not changed.  Returns self.
        ValueError: a source that is no model on the device, that is this view, that belongs to another parent or that is in the
        middle of a streamed run(); a parent whose engine was re-created."""
        self._check_parent()
        if source is None:
            source = self._parent()
            if source is None:
                raise ValueError("sync(): the parent model is gone; name the view to continue")
        if not isinstance(source, HierarchicalTemporalMemory) or source._engine is None:
            raise ValueError("sync(): the source must be a model with both layers on the device")
        if source is self:
            raise ValueError("sync(): a view cannot be synced to itself")
        if isinstance(source, InferenceView):
            source._check_parent()
            owner = source._parent_engine()
        else:
            owner = source._engine
        if owner is not self._parent_engine():          # (both gone: the library compares the weights the handles share)
            raise ValueError("sync(): the source belongs to another parent (a view continues its parent or a view of the same parent)")
        if source._streaming or self._streaming:
            raise ValueError("sync(): the source or the view is in the middle of a streamed run() (continuing=True): end the stream first")
        retire_states(self._engine)
        try:
            self._engine.view_sync(source._engine)
        except HtmError as e:                       # (what only the library can tell: two views whose parent is gone)
            raise ValueError(f"sync(): {e}") from e
        mine, theirs = self.temporal_memory, source.temporal_memory
        mine._last_ref, mine._host_last = None, None
        mine._last_cols, mine._was_reset = theirs._last_cols, theirs._was_reset
        return self

    def fork(self):
        """A sibling view that continues THIS view's stream (a branch of a what-if stream): a new view of the parent, synced to
        this view.  ValueError when the parent model is gone."""
        self._check_parent()
        parent = self._parent()
        if parent is None:
            raise ValueError("fork() of a view: the parent model is gone (new views are made of the model that owns the weights)")
        try:
            view = parent.inference_view()
        except HtmError as e:                       # (the parent has a step open phase by phase)
            raise ValueError(f"fork(): {e}") from e
        return view.sync(self)

    def _forkable_engine(self, what):
        self._check_parent()
        if self._parent() is None:
            raise ValueError(f"{what} of a view: the parent model is gone (new views are made of the model that owns the weights)")
        if self._streaming:
            raise ValueError(f"{what}: this view is in the middle of a streamed run() (continuing=True): end the stream first")
        return self._engine

    def lookahead(self, inputs, steps, horizon, min_votes=1, max_bits=0, every=1, learning=False, use_graph=True, record=None,
                  resets=None, noise=0.0, noise_seed=None, encoder=None):
        self._no_learning(learning, "lookahead()")
        self._check_parent()
        return super().lookahead(inputs, steps, horizon, min_votes, max_bits, every=every, learning=False, use_graph=use_graph,
                                 record=record, resets=resets, noise=noise, noise_seed=noise_seed, encoder=encoder)

    def inference_view(self):
        raise ValueError("inference_view() of a view: make views of the model that owns the weights")

    def state_dict(self):
        raise ValueError("state_dict() of an inference view: it shares its parent's weights; save the parent instead")

    def save(self, path):
        raise ValueError("save() of an inference view: it shares its parent's weights; save the parent instead")

    def load_state_dict(self, state):
        raise ValueError("load_state_dict() on an inference view: load the parent and make new views")

    def load(self, path):
        raise ValueError("load() on an inference view: load the parent and make new views")

    def grow_pool(self, segment_capacity=None, segment_slots=None):
        raise ValueError("grow_pool() on an inference view: its pool is its parent's; grow the parent and make new views")


def _cached_bank(owner, eng, inputs, fresh=False, encoder=None):
    """The device bank of `inputs` (bool [n, input_dim]) on `eng`: uploaded once and kept on `owner` until the inputs change
    (fresh: uploaded again -- a new engine).  With an `encoder`, `inputs` are its values (float64 [n, F]): uploaded as they
    are and encoded on the device (Engine.encoded_bank), cached in the same way."""
    key = (inputs.shape, inputs.tobytes()) if encoder is None else (inputs.shape, inputs.tobytes(), encoder.key())
    bank = getattr(owner, "_bank", None)
    if fresh or bank is None or bank[0] != key:
        owner._bank = bank = (key, eng.upload_bank(inputs) if encoder is None else eng.encoded_bank(encoder, inputs))
    return bank[1]


def _noise_ring(owner, eng, chunk):
    """(ring bank, its reset bits, rows) of run(noise=) on `eng`: chunk + 2 rows at a fixed address, so that the graphs of the runs
    over it, which are keyed by the bank, are captured once; kept on `owner` until its engine is re-created (as _zero_bank)."""
    rows = int(chunk) + 2
    if rows < 3:
        raise ValueError(f"noise_chunk must be at least 1, got {chunk}")
    rings = getattr(owner, "_noise_rings", None)
    if rings is None or rings[0]() is not eng:
        owner._noise_rings = rings = (weakref.ref(eng), {})
    if rows not in rings[1]:
        rings[1][rows] = (eng.zero_bank(rows), eng.zero_resets(rows), rows)
    return rings[1][rows]


def _with_counters(record):
    """run(record=..., likelihood=): the record with the counters the likelihood reads."""
    if record is None or record is True:
        return True
    fields = (record,) if isinstance(record, str) else tuple(record)
    return fields if "counters" in fields else ("counters",) + fields


def _no_classifier(classifier, what):
    """The calls an SDRClassifier does not ride on: refused, never silently ignored."""
    if classifier is not None:
        raise ValueError(f"{what}: classifier= is not available here -- an SDRClassifier rides on HierarchicalTemporalMemory.run() and "
                         "InferenceView.run(), or takes patterns through update_patterns(); ModelGroup.run() and tick() take an "
                         "SDRClassifierBank of as many streams as the group has members")


def _no_knn(knn, what):
    """The calls a KNNClassifier does not ride on: refused, never silently ignored."""
    if knn is not None:
        raise ValueError(f"{what}: knn= is not available here -- a KNNClassifier rides on HierarchicalTemporalMemory.run() and "
                         "InferenceView.run(), or takes patterns through update_patterns(); ModelGroup.run() and tick() take a KNNClassifierBank of as "
                         "many streams as the group has members")


def _classifier_targets(classifier, targets, inputs, encoder):
    """run(classifier=, targets=): the target bucket of every row of `inputs` -> int32 [rows]."""
    if targets is None:
        if encoder is None or classifier.field is None:
            raise ValueError("run(classifier=): give targets=, or encoder= and a classifier made with field=")
        where = [j for j, f in enumerate(encoder.fields) if f is classifier.field]
        if not where:
            raise ValueError("run(classifier=): the classifier's field is not one of the encoder's fields")
        targets = encoder.bucket(inputs)[:, where[0]]
    targets = classifier.check_targets(targets)
    if targets.shape != (inputs.shape[0],):
        raise ValueError(f"targets: one bucket per row of inputs ({inputs.shape[0]}), got {targets.shape[0]}")
    return targets


def _join_record(parts, fields, first_step, steps, k, column_dim, input_dim=0, encoder=None, likelihood=False, classifier=None, knn=None):
    """One contiguous RunRecord from the per-batch records of a run(record=...) (Engine.run's dicts), however many batches the
    pool's growth cut the call into."""
    empty = {"counters": np.zeros((0, len(RECORD_COUNTERS)), np.int32), "active_column": np.zeros((0, k), np.int32),
             "column_prediction": np.zeros((0, (column_dim + 31) // 32), np.uint32), "predicted_input": np.zeros((0, input_dim), np.int32),
             "predicted_value": np.zeros((0, 2 * len(encoder or ())), np.int32)}
    whole = {f: np.concatenate([p[f] for p in parts]) if parts else empty[f] for f in fields}
    if "predicted_value" in whole:                  # (bucket, score) pairs per field -> the record's three arrays
        pairs = whole.pop("predicted_value").reshape(steps, len(encoder), 2)
        bucket = np.ascontiguousarray(pairs[:, :, 0])
        whole.update(predicted_bucket=bucket, predicted_score=np.ascontiguousarray(pairs[:, :, 1]), predicted_value=encoder.value_of(bucket))
    if "column_prediction" in whole:
        words = np.ascontiguousarray(whole["column_prediction"])
        whole["column_prediction"] = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :column_dim].astype(bool)
    if likelihood:                                  # (each batch's part carries its steps' likelihoods beside the fields)
        whole["anomaly_likelihood"] = np.concatenate([p["anomaly_likelihood"] for p in parts]) if parts else np.zeros(0, np.float64)
    if classifier is not None:                      # (each batch's part carries its steps' predictions beside the fields)
        H = len(classifier.steps)
        whole["classified"] = np.concatenate([p["classified"] for p in parts]) if parts else np.zeros((0, H, 2), np.int32)
        if parts and parts[0]["class_distribution"] is not None:
            whole["class_distribution"] = np.concatenate([p["class_distribution"] for p in parts])
        whole["classified_field"] = classifier.field
    if knn is not None:                             # (likewise: each batch's part carries its steps' result rows)
        whole["knn"] = np.concatenate([p["knn"] for p in parts]) if parts else np.zeros((0, 5), np.int32)
        if parts and parts[0]["knn_votes_all"] is not None:
            whole["knn_votes_all"] = np.concatenate([p["knn_votes_all"] for p in parts])
    return RunRecord(first_step + np.arange(steps, dtype=np.int64), **whole)


def batch_steps(left, free_segments=None, per_step=1, cap=None, period=1, multiple=1):
    """Steps the next device-side batch of a run may take, of `left` that remain: what `free_segments` free segments are expected
    to last at `per_step` new segments per step of the model (2 x active columns: every column bursting, twice), less one.  The
    model steps once per `period` steps of the run, and the answer is a multiple of `multiple`, at least one (the run must get
    on: a pool that overflows inside the batch is reported, never silent).  None free segments: a pool nobody looks at, no limit.
    `cap`: a limit of the caller's own (the steps per noise ring, per forecast bank, per chunk of a stack)."""
    if free_segments is not None:
        left = min(left, max(multiple, (free_segments // per_step - 1) * period // multiple * multiple))
    return left if cap is None else min(left, cap)


def _looked_at_pool(model, per_step, refuse=None, regrown=None):
    """The pool step between two batches of a run on `model` (a HierarchicalTemporalMemory or a TemporalMemory): check, grow,
    check again -> its engine's free segments, or None for a pool that does not grow.  `refuse`: why the pool must not grow now
    (RuntimeError).  `regrown()`: what the caller has to upload again once model._engine is a new engine."""
    eng = model._engine
    if not eng._auto_grow:
        return None
    if eng.pool_look(per_step, force=True):
        if refuse:
            raise RuntimeError(refuse)
        model.grow_pool(*eng._grow_to)
        eng = model._engine
        if regrown is not None:
            regrown()
        eng.pool_look(per_step, force=True)
    return eng._free_segments


def _batches(steps, pools=None, cap=None, multiple=1):
    """(steps done, steps of the next batch) until `steps` are done.  `pools()`, called before every batch, looks at the pools the
    batch draws on -- growing them first where that is due -- and yields (free segments, per_step, period) for each
    (batch_steps); None: nobody looks.  What pools() returns is always consumed in full before the batch is handed out: a
    generator may do work of its own between two pools and behind the last (the stack uploads level 0's bank again there).
    `cap`, `multiple`: batch_steps'."""
    done = 0
    while done < steps:
        n = batch_steps(steps - done, cap=cap)
        for free, per_step, period in (pools() if pools is not None else ()):
            n = batch_steps(n, free, per_step, period=period, multiple=multiple)
        yield done, n
        done += n


class _BatchedCall:
    """The records and the tail of one batched call over the Temporal Memories `tms` (a fused model's temporal_memory shares
    the model's engine): the parts every batch adds per member, the step each started at, and at the end the new last_state, the
    sticky flags and one RunRecord per member."""

    def __init__(self, tms, fields, encoder=None, likelihood=False, classifier=None, knn=None):
        self.tms, self.fields, self.encoder, self.likelihood, self.classifier, self.knn = tms, fields, encoder, likelihood, classifier, knn
        self.first = [tm._engine.steps for tm in tms]
        self.parts = [[] for _ in tms]

    def add(self, parts):
        """One batch's record dictionaries, one per member (ignored in a call without a record)."""
        if self.fields is not None:
            for mine, part in zip(self.parts, parts):
                mine.append(part)

    def finish(self, steps, ks, columns=None, read=None):
        """`steps`, `ks`: per member, the steps it took and the width of its "active_column" rows; `columns`: per member, the
        active columns its last step was given (None: the device's own, of a fused model; no entry: no new last_state);
        `read()`: for a caller whose records stay on the device until the end, what add() takes, read after the wait."""
        for tm, cols in zip(self.tms, [None] * len(self.tms) if columns is None else columns):
            tm._new_state(cols)
        for tm in self.tms:
            tm._engine.check_capacity()
        if self.fields is None:
            return [None] * len(self.tms)
        if read is not None:
            self.add(read())
        return [_join_record(p, self.fields, f, n, k, tm.column_dim, tm._engine.input_dim, self.encoder, self.likelihood, self.classifier, self.knn)
                for p, f, n, k, tm in zip(self.parts, self.first, steps, ks, self.tms)]
