"""Region stacks: regions on top of each other, each reading the active columns of the one below (DESIGN.md section 14;
include/bithtm_hip.h, htm_pack_columns).

In reference terms a stack of L levels is L HierarchicalTemporalMemory objects with input_dim[l + 1] == column_dim[l].  Level 0
steps on every input; level l + 1 makes its step u after level l has finished its steps u * s_l .. (u + 1) * s_l - 1 (s_l: the
link's stride, default 1), on the bool vector with a bit for every column in sp_state.active_column of any step of that window.
Level l draws with seed + l.  Nothing flows downwards.

    stack = RegionStack(1000, [(65536, 32), (8192, 32)], strides=[4])
    stack.run(inputs, 2000)                       # the device path: no host work between the levels
    sp1, tm1 = stack.process(x)[1] or (None, None)  # the reference's loop, through the host: None in the middle of a window
    stack.levels[1].predicted_input()             # the levels stay ordinary models for reading

A link is plain (the OR above; an int in `links=` is its stride) or a pooling link (pooling.PoolingLink): the
upper level then reads the union_bits lower columns of the largest persistence, a decaying union that stays put while the lower
level is inside a sequence it knows.  A pooling link has a state (persistence and the lower level's last column prediction).  It
lives on the HOST between calls (stack.link_state(l)): process() steps it there with the NumPy definition, run() copies it to the
device before its first launch, htm_pool_columns carries it through the call's chunks on the device, and run() reads it back behind
the one synchronisation at its end -- so process() and run() mix freely.

    stack = RegionStack(1000, [(65536, 32), (8192, 32)], links=[PoolingLink(stride=4)])
"""

import os

import numpy as np

from . import _lib as L
from .engine import words_to_bool
from .group import SharedStream
from .pooling import PoolingLink, PoolingState
from .networks import HierarchicalTemporalMemory, InferenceView, _BatchedCall, _batches, _cached_bank, _check_encoder, _looked_at_pool, _record_fields, retire_states

CHUNK_STEPS = 2048              # level-0 steps per chunk of run() (BITHTM_STACK_CHUNK; rounded down to a multiple of the strides' product)


def _refuse_level(i, m):
    """Why model i cannot be a level of a stack (ValueError), or None."""
    if isinstance(m, InferenceView):
        return f"level {i} is an inference view (a stack's levels learn; stacks of views are not available)"
    if not isinstance(m, HierarchicalTemporalMemory):
        return f"level {i} is a {type(m).__name__}, not a HierarchicalTemporalMemory (column-sharded models cannot be stacked)"
    if getattr(m.temporal_memory, "cell_dim", m.cell_dim) > 64 or m.cell_dim > 64:
        return f"level {i} has cell_dim {m.cell_dim} > 64: its Temporal Memory steps on the host"
    if m.engine is None or not getattr(m.spatial_pooler, "_plain", False):
        return f"level {i} has a layer, a distal projection or plug-in objects that live on the host"
    if m.engine.shard_world > 1:
        return f"level {i} is column-sharded"
    if m._streaming:
        return f"level {i} is in the middle of a streamed run() (continuing=True): end the stream first"
    return None


def _check_strides(strides, links):
    strides = [1] * links if strides is None else [int(s) for s in strides]
    if len(strides) != links or any(s < 1 for s in strides):
        raise ValueError(f"strides: {links} integers >= 1 (one per link between two levels), got {strides}")
    return strides


def _check_links(strides, links, n):
    """`strides=` or `links=` of a stack with n links -> a list of n entries, each an int (a plain link's stride) or a PoolingLink."""
    if links is None:
        return _check_strides(strides, n)
    if strides is not None:
        raise ValueError("give strides= or links=, not both (an int in links= is a plain link's stride)")
    links = list(links)
    if len(links) != n or any(isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer, PoolingLink)) for k in links):
        raise ValueError(f"links: {n} entries (one per link between two levels), each an int (a stride) or a PoolingLink, got {links}")
    plain = [int(k) for k in links if not isinstance(k, PoolingLink)]
    if any(k < 1 for k in plain):
        raise ValueError(f"links: strides are integers >= 1, got {plain}")
    return [k if isinstance(k, PoolingLink) else int(k) for k in links]


def _resolve(link, l, column_dim, active_columns):
    """The pooling link l over its lower level (PoolingLink.resolved: union_bits filled in and checked)."""
    if active_columns is None:                      # (the models' default: HierarchicalTemporalMemory's active_columns)
        active_columns = max(1, round(column_dim * 0.02))
    try:
        return link.resolved(column_dim, active_columns)
    except ValueError as e:
        raise ValueError(f"link {l}: {e}") from None


def _check_shape(input_dim, levels, strides, links):
    """The constructor's arguments of a stack -> (levels as tuples of ints, the links as _check_links returns them); every
    ValueError of a shape that cannot be built, before anything touches a device."""
    levels = [tuple(int(v) for v in lv) for lv in levels]
    if not levels or any(len(lv) not in (2, 3) for lv in levels):
        raise ValueError("levels: a non-empty list of (column_dim, cell_dim) or (column_dim, cell_dim, active_columns)")
    links = _check_links(strides, links, len(levels) - 1)
    for i, lv in enumerate(levels):
        if lv[0] < 1 or lv[1] < 1 or (len(lv) == 3 and not 1 <= lv[2] <= lv[0]):
            raise ValueError(f"level {i}: column_dim and cell_dim >= 1, 1 <= active_columns <= column_dim (got {lv})")
        if lv[1] > 64:
            raise ValueError(f"level {i} has cell_dim {lv[1]} > 64: its Temporal Memory steps on the host")
    if int(input_dim) < 1:
        raise ValueError(f"input_dim must be at least 1 (got {input_dim})")
    for i, link in enumerate(links):            # (a pooling link that does not fit its lower level: before anything touches a device)
        if isinstance(link, PoolingLink):
            _resolve(link, i, levels[i][0], levels[i][2] if len(levels[i]) == 3 else None)
    return levels, links


class RegionStack:
    """L fused HierarchicalTemporalMemory models chained through their active columns (see the module's docstring).  `levels`:
    a list of (column_dim, cell_dim) or (column_dim, cell_dim, active_columns), bottom first; `strides`: one per link.  All
    levels enqueue on ONE stream (so each keeps its fastest schedule, and the device path needs no events between them)."""

    def __init__(self, input_dim, levels, strides=None, seed=0, device=0, links=None):
        levels, links = _check_shape(input_dim, levels, strides, links)
        stream = SharedStream(device)
        models, below = [], int(input_dim)
        for i, lv in enumerate(levels):
            models.append(HierarchicalTemporalMemory(below, lv[0], lv[1], active_columns=lv[2] if len(lv) == 3 else None,
                                                     seed=int(seed) + i, device=device, stream=stream))
            below = lv[0]
        self._setup(models, links)

    @classmethod
    def of(cls, models, strides=None, links=None):
        """A stack over existing fused models, bottom first.  ValueError if the dims do not chain (input_dim of a level is not
        the column_dim of the one below), if a model has plug-in objects on the host, cell_dim above 64, is column-sharded, an
        inference view or in a streamed run, or if the models do not share one stream (ModelGroup.create and
        HierarchicalTemporalMemory(stream=) make models that do)."""
        models = list(models)
        if not models:
            raise ValueError("a region stack needs at least one level")
        links = _check_links(strides, links, len(models) - 1)
        for i in range(1, len(models)):
            lower = getattr(models[i - 1], "column_dim", None)
            upper = getattr(getattr(models[i], "spatial_pooler", None), "input_dim", None)
            if lower is not None and upper is not None and lower != upper:
                raise ValueError(f"level {i}: input_dim {upper} is not level {i - 1}'s column_dim {lower}")
        for i, m in enumerate(models):
            why = _refuse_level(i, m)
            if why:
                raise ValueError(why)
            if any(models[j] is m for j in range(i)):
                raise ValueError(f"level {i} is a lower level again")
        for i in range(1, len(models)):
            if models[i].engine.input_dim != models[i - 1].column_dim:
                raise ValueError(f"level {i}: input_dim {models[i].engine.input_dim} is not level {i - 1}'s column_dim {models[i - 1].column_dim}")
        s0 = models[0].engine.stream_handle()
        for i, m in enumerate(models):
            if m.engine.stream_handle() != s0 or m.engine.device != models[0].engine.device:
                raise ValueError(f"level {i} enqueues on another stream than level 0: create the models on one stream "
                                 "(HierarchicalTemporalMemory(stream=...), ModelGroup.create)")
        self = cls.__new__(cls)
        self._setup(models, links)
        return self

    def _setup(self, models, links):
        self.levels = models
        # links[l]: the link between the levels l and l + 1 -- an int (a plain link's stride) or a PoolingLink with its union_bits filled in
        self.links = [_resolve(k, l, models[l].column_dim, models[l].active_columns) if isinstance(k, PoolingLink) else k for l, k in enumerate(links)]
        self.strides = [k.stride if isinstance(k, PoolingLink) else k for k in self.links]
        self._pool = {l: PoolingState(k, models[l].column_dim) for l, k in enumerate(self.links) if isinstance(k, PoolingLink)}
        self.pool_scratch_bytes = L.POOL_SCRATCH_BYTES      # run(): the most scratch a pooling link's calls get (fewer bytes: more batches)
        self._period = [1]                          # level-0 steps per step of level l
        for s in self.strides:
            self._period.append(self._period[-1] * s)
        self._S = self._period[-1]
        self._steps = 0                             # the stack's own step counter: windows are counted from it, nothing resets it
        self._window = [np.zeros(m.column_dim, dtype=np.bool_) for m in models[:-1]]     # process(): the open window of each link
        self.chunk_steps = int(os.environ.get("BITHTM_STACK_CHUNK", CHUNK_STEPS))
        self.lib = L.load()
        self._bufs = {}                             # run(): device buffers {(level, name): (address, 32-bit words)}
        self.last_run_chunks = []                   # run(), diagnostic: (level-0 steps, graph_count() of every level) after each chunk

    def __len__(self):
        return len(self.levels)

    def __del__(self):
        bufs, self._bufs = getattr(self, "_bufs", {}), {}
        if bufs:
            for m in getattr(self, "levels", []):
                if m.engine is not None and m.engine.h:
                    m.engine.sync()
            for ptr, _ in bufs.values():
                self.lib.hipFree(ptr)

    @property
    def steps(self):
        """Inputs the stack has processed (process() calls and run() steps)."""
        return self._steps

    # ---- the reference's loop
    def process(self, x, learning=True):
        """One input: level 0 steps, and every upper level whose window this step completes.  Returns a list with one entry per
        level: (sp_state, tm_state) for the levels that stepped, None for the levels in the middle of a window.

        This is the reference's own loop and it goes through the host between the levels: it reads each level's active columns
        back, ORs them into a host accumulator and calls the next level's process().  It is the convenience path and the
        parity yardstick of run(), not the fast path: run() keeps the whole loop on the device."""
        self._check_levels()
        out = [None] * len(self.levels)
        for l, m in enumerate(self.levels):
            out[l] = m.process(x, learning=learning)
            if l + 1 == len(self.levels):
                break
            active = m.engine.read(L.F_ACTIVE_COLUMN, np.int32, m.engine.active_columns)
            pool = self._pool.get(l)
            if pool is not None:                    # (a pooling link steps whatever `learning` is: it is dynamics, not weights)
                pool.step(active, words_to_bool(m.engine.read(L.F_CELL_PREDICTION, np.uint32, m.engine.cell_words), m.cell_dim).any(axis=1))
            window = self._window[l]
            if pool is None:
                window[active] = True
            if (self._steps + 1) % self._period[l + 1]:
                break                               # (the window of the link above is still open)
            x = window.copy() if pool is None else pool.row()
            window[:] = False
        self._steps += 1
        return out

    compute = process

    def reset(self):
        """A sequence reset of EVERY level before the next input (HierarchicalTemporalMemory.reset).  Only between windows: when
        the steps taken are a multiple of the product of the strides (ValueError otherwise)."""
        if self._steps % self._S:
            raise ValueError(f"reset(): the stack has taken {self._steps} steps, not a multiple of {self._S} (the product of the "
                             "strides): an upper level is in the middle of a window")
        for m in self.levels:
            m.reset()
        for pool in self._pool.values():
            pool.reset()

    def link_state(self, l):
        """(persistence uint8[C], prev bool[C]) of the pooling link between the levels l and l + 1 (copies; ValueError for a
        plain link)."""
        if l not in self._pool:
            raise ValueError(f"link {l} is not a pooling link")
        return self._pool[l].persistence.copy(), self._pool[l].prev.copy()

    # ---- the device path
    def _check_levels(self):
        for i, m in enumerate(self.levels):
            if m._streaming:
                raise ValueError(f"level {i} is in the middle of a streamed run() (continuing=True): end the stream first")

    def _buffer(self, level, name, words):
        """Device address of the stack's buffer (level, name) of at least `words` 32-bit words (kept, made anew when too small;
        one stream: level 0's engine waits for everything that used the old one)."""
        return self.levels[0].engine.kept_buffer(self._bufs, (level, name), words)

    def run(self, inputs, steps, learning=True, use_graph=True, record=None, resets=None):
        """`steps` inputs from the rows of the boolean matrix `inputs`, cycled (as HierarchicalTemporalMemory.run), through all
        levels on the device: per chunk of at most `chunk_steps` level-0 steps, level 0 runs recorded (its active columns stay
        in device memory), htm_pack_columns packs them into level 1's bank, level 1 runs over it, and so on -- one stream, no
        host wait inside a chunk.  The state every level is left in equals that of the same inputs given one by one to
        process().  `steps` and the steps taken so far must be multiples of the product of the strides (ValueError): no
        half-filled window is carried across calls.
        `record`: as HierarchicalTemporalMemory.run; the call then returns one RunRecord per level (level l's over its
        steps / (s_0 .. s_{l-1}) steps), read back after one synchronisation at the end of the call.
        `resets`: a bool per row of `inputs`: a sequence reset of every level before each step that reads a flagged row.  Flagged
        rows must be multiples of the strides' product, and the number of rows must divide by it when steps exceeds it, so
        that every reset stands on a window boundary of every level (ValueError otherwise)."""
        S, nl = self._S, len(self.levels)
        steps = int(steps)
        if steps < 0 or steps % S or self._steps % S:
            raise ValueError(f"run(): steps ({steps}) and the steps taken so far ({self._steps}) must be multiples of {S}, the product "
                             "of the strides")
        self._check_levels()
        fields = None if record is None else _record_fields(record)
        _check_encoder(None, fields, 0, 0)          # (a stack takes no encoder: "predicted_value" is a ValueError)
        m0 = self.levels[0]
        inputs = np.asarray(inputs, dtype=np.bool_)
        if inputs.ndim != 2 or inputs.shape[0] < 1 or inputs.shape[1] != m0.engine.input_dim:
            raise ValueError(f"inputs: bool [n_inputs, {m0.engine.input_dim}], got {inputs.shape}")
        n_rows = inputs.shape[0]
        flags = None                                # flags[i]: a reset before the i-th step of this call
        if resets is not None:
            resets = np.asarray(resets, dtype=np.bool_).ravel()
            if resets.shape != (n_rows,):
                raise ValueError(f"resets: one flag per row of inputs ({n_rows}), got {resets.shape[0]}")
            flagged = np.flatnonzero(resets)
            if (flagged % S).any():
                raise ValueError(f"resets: flagged rows must be multiples of {S}, the product of the strides (got rows {flagged[flagged % S != 0][:8].tolist()})")
            if flagged.size and steps > n_rows and n_rows % S:
                raise ValueError(f"resets: {steps} steps cycle through {n_rows} rows, which is not a multiple of {S} (the product of the "
                                 "strides): the cycled flags would leave the window boundaries")
            i = np.arange(steps, dtype=np.int64)
            flags = resets[(m0.engine.steps + i) % n_rows]
            if ((self._steps + i)[flags] % S).any():
                raise ValueError(f"resets: a flagged row is read at a stack step that is not a multiple of {S} (level 0 has taken "
                                 f"{m0.engine.steps} steps, the stack {self._steps})")
        for m in self.levels:
            retire_states(m.engine)
        period = self._period
        chunk = max(S, min(max(self.chunk_steps, 1), max(steps, 1)) // S * S)
        shapes = [m.engine.record_shapes() for m in self.levels]
        # what each level records: the user's fields over the whole call (read back at its end), and, below another level, its
        # active columns -- over one chunk if the user did not ask for them
        rows = []
        for l, m in enumerate(self.levels):
            want = dict.fromkeys(fields or (), steps // period[l])
            if l + 1 < nl:
                want.setdefault("active_column", chunk // period[l])
                if l in self._pool:                 # (a pooling link reads what the step predicted, too)
                    want.setdefault("column_prediction", chunk // period[l])
            rows.append(want)
        pools = {l: self._pool_buffers(l, chunk // period[l + 1]) for l in self._pool if steps}
        self.last_run_chunks = []
        bank = _cached_bank(m0, m0.engine, inputs)
        call = _BatchedCall([m.temporal_memory for m in self.levels], fields)

        def segment_pools():                        # default-sized pools grow as in single-model runs: a look between chunks
            nonlocal bank
            for l, m in enumerate(self.levels):
                eng = m.engine
                yield _looked_at_pool(m, 2 * m.active_columns), 2 * m.active_columns, period[l]
                if l == 0 and m.engine is not eng:  # (_batches comes back here before the chunk runs: level 0's bank on its new engine)
                    bank = _cached_bank(m0, m.engine, inputs, fresh=True)
        for done, n in _batches(steps, segment_pools, cap=chunk, multiple=S):
            below = below_pred = None               # device addresses of the lists (and the column predictions) of the level below, this chunk
            for l, m in enumerate(self.levels):
                eng = m.engine
                n_l, done_l = n // period[l], done // period[l]
                bufs = {}
                for f, total in rows[l].items():
                    w = shapes[l][f][0]
                    whole = fields is not None and f in fields
                    bufs[f] = self._buffer(l, f, max(total, 1) * w) + (4 * done_l * w if whole else 0)
                if l == 0:
                    level_bank, bank_rows = bank, n_rows
                    bits = None if resets is None else eng.upload_resets(resets)
                else:
                    # (a run reads bank row step_index % n_inputs of ITS handle: the chunk's rows start at that row)
                    level_bank, bank_rows = self._buffer(l, "bank", (chunk // period[l]) * eng.words), n_l
                    first_row = eng.steps % n_l
                    lower = self.levels[l - 1]
                    bits = None
                    if flags is not None:           # a flag on a level-0 step = a flag on the upper step whose window starts there
                        row_flags = np.zeros(n_l, dtype=np.bool_)
                        row_flags[(first_row + np.arange(n_l)) % n_l] = flags[done:done + n:period[l]]
                        bits = eng.upload_resets(row_flags)
                    if l - 1 in pools:              # (the link's reset bits are the upper level's: one per window = per bank row)
                        persistence, prev, scratch, scratch_bytes = pools[l - 1]
                        eng.pool_columns(self.links[l - 1], below, lower.active_columns, below_pred, n_l, persistence, prev, bits, scratch, scratch_bytes,
                                         level_bank, n_l, first_row)
                    else:
                        eng.pack_columns(below, lower.active_columns, n_l, self.strides[l - 1], level_bank, n_l, first_row)
                with eng.this_call(bits, bank_rows):
                    # (no HTM_RUN_CONTINUE: an upper level working ahead would read a row of the next chunk before it is packed,
                    # and every level is at rest between chunks, where the pools are looked at)
                    eng.run_into(level_bank, bank_rows, n_l, bufs, learning=learning, use_graph=use_graph)
                m._streaming = False
                below, below_pred = bufs.get("active_column"), bufs.get("column_prediction")
            self._steps += n
            self.last_run_chunks.append((n, tuple(m.engine.graph_count() for m in self.levels)))
        totals = [steps // p for p in period]
        if pools:                                   # the links' state comes home behind the call's one wait
            m0.engine.sync()
            for l, (persistence, prev, _, _) in pools.items():
                C = self._pool[l].column_dim
                self._pool[l].persistence[:] = m0.engine.read_words(persistence, (C + 3) // 4, np.uint32).view(np.uint8)[:C]
                self._pool[l].prev[:] = np.unpackbits(m0.engine.read_words(prev, (C + 31) // 32, np.uint32).view(np.uint8), bitorder="little")[:C]

        def read():                                 # (after finish() has synchronised: an overflow is reported by the call it happened in)
            return [{f: m0.engine.read_words(self._bufs[(l, f)][0], n * shapes[l][f][0], shapes[l][f][1]).reshape(n, shapes[l][f][0]) for f in fields}
                    for l, n in enumerate(totals)]
        records = call.finish(totals, [m.active_columns for m in self.levels], read=read)
        return None if fields is None else records

    def _pool_buffers(self, l, windows):
        """The device side of the pooling link l for a run() whose chunks hold at most `windows` of its windows: (persistence, prev,
        scratch, scratch bytes), the state arrays holding the host's state.  Called before the call's first launch: the stream is
        at rest (every run() ends with a wait), so the copies order themselves."""
        pool, lower, upper = self._pool[l], self.levels[l], self.levels[l + 1]
        C = pool.column_dim
        if C > L.POOL_MAX_COLUMNS:
            raise ValueError(f"link {l}: a pooling link serves at most {L.POOL_MAX_COLUMNS} lower columns on the device (level {l} has {C})")
        window = (pool.link.stride + 8) * 4 * upper.engine.words           # (htm_pool_columns: a window's bitmap rows and its snapshot row)
        if window > self.pool_scratch_bytes:
            raise ValueError(f"link {l}: one window needs {window} bytes of scratch, above the bound of {self.pool_scratch_bytes} (pool_scratch_bytes)")
        scratch_bytes = min(self.pool_scratch_bytes // window, max(windows, 1)) * window
        persistence = self._buffer(l, "pool_persistence", (C + 3) // 4)
        prev = self._buffer(l, "pool_prev", (C + 31) // 32)
        scratch = self._buffer(l, "pool_scratch", (scratch_bytes + 3) // 4)
        eng = lower.engine
        for ptr, data in ((persistence, pool.persistence), (prev, np.packbits(pool.prev, bitorder="little"))):
            data = np.ascontiguousarray(data)
            eng._hip_check(self.lib.hipMemcpy(ptr, data.ctypes.data, data.nbytes, L.HIP_MEMCPY_HOST_TO_DEVICE), "hipMemcpy")
        return persistence, prev, scratch, scratch_bytes

    # ---- checkpoints
    def state_dict(self):
        """The levels' own dictionaries under the prefixes l0_, l1_, ..., with `stack_steps`, `strides` and the open window of
        every link (`link<l>_window`: all False between windows)."""
        out = {}
        for l, m in enumerate(self.levels):
            out.update({f"l{l}_{k}": v for k, v in m.state_dict().items()})
        out["stack_steps"] = np.int64(self._steps)
        out["strides"] = np.asarray(self.strides, dtype=np.int64)
        for l, w in enumerate(self._window):
            if l in self._pool:                     # a pooling link: its parameters and its state (it keeps no window)
                out[f"link{l}_parameters"] = self.links[l].as_array()
                out[f"link{l}_persistence"], out[f"link{l}_prev"] = self.link_state(l)
            else:
                out[f"link{l}_window"] = w.copy()
        return out

    def load_state_dict(self, state):
        """ValueError if the dictionary is of a stack of other shapes, strides or links."""
        strides = np.asarray(state.get("strides", ()), dtype=np.int64).ravel().tolist() if "strides" in state else None
        if strides != self.strides or "stack_steps" not in state:
            raise ValueError(f"load_state_dict(): the state's strides {strides} are not this stack's {self.strides}")
        parts = []
        for l, m in enumerate(self.levels):
            part = {k[len(f"l{l}_"):]: v for k, v in state.items() if k.startswith(f"l{l}_")}
            perm, pred = part.get("sp_permanence"), part.get("tm_prev_prediction")
            want = (m.column_dim, m.engine.input_dim)
            if perm is None or pred is None or tuple(np.shape(perm)) != want or tuple(np.shape(pred)) != (m.column_dim, m.cell_dim):
                raise ValueError(f"load_state_dict(): level {l} of the state is not {want[1]} -> {m.column_dim} x {m.cell_dim}")
            parts.append(part)
        for l in range(len(self.links)):
            got = np.asarray(state[f"link{l}_parameters"]).ravel().tolist() if f"link{l}_parameters" in state else None
            want = self.links[l].as_array().tolist() if l in self._pool else None
            if got != want:
                raise ValueError(f"load_state_dict(): link {l} of the state ({'plain' if got is None else got}) is not this stack's "
                                 f"({'plain' if want is None else self.links[l]})")
            if want is not None:
                C = self._pool[l].column_dim
                if any(np.shape(state.get(f"link{l}_{name}")) != (C,) for name in ("persistence", "prev")):
                    raise ValueError(f"load_state_dict(): link {l} of the state has no persistence and prev of {C} columns")
        if any(k.startswith(f"l{len(self.levels)}_") for k in state):
            raise ValueError(f"load_state_dict(): the state has more than this stack's {len(self.levels)} levels")
        for m, part in zip(self.levels, parts):
            m.load_state_dict(part)
        self._steps = int(state["stack_steps"])
        for l, w in enumerate(self._window):
            w[:] = np.asarray(state[f"link{l}_window"], dtype=np.bool_) if f"link{l}_window" in state else False
        for l, pool in self._pool.items():
            pool.persistence[:] = np.asarray(state[f"link{l}_persistence"], dtype=np.uint8)
            pool.prev[:] = np.asarray(state[f"link{l}_prev"], dtype=np.bool_)

    def save(self, path):
        np.savez_compressed(path, **self.state_dict())

    def load(self, path):
        with np.load(path) as z:
            self.load_state_dict({k: z[k] for k in z.files})

