"""Stacks of model groups: B independent streams through one hierarchy, every launch covering all of them (DESIGN.md section 30;
include/bithtm_hip.h, htm_group_pack_columns and htm_group_pool_columns).

A GroupStack is to a RegionStack (stack.py) what a ModelGroup (group.py) is to a model: member b is a RegionStack of its own --
levels, links, link states, step counter -- and a GroupStack call leaves it as if it had made the call itself; but level l of ALL
members is one ModelGroup, and the link between two levels is one htm_group_pack_columns / htm_group_pool_columns call, so the
launches of a chunk do not depend on B.

    stack = GroupStack(64, 1000, [(2048, 32), (512, 32)], strides=[4])
    stack.run(inputs, 2000)                       # inputs: bool [64, n_inputs, 1000]; stream b cycles through inputs[b]
    stack.process(X)                              # X: bool [64, 1000], the stepwise loop through the host
    GroupStack.of(stacks)                         # B existing RegionStacks on one stream, stepped together from now on
    GroupStack.views(trained, 16)                 # 16 streams over ONE copy of a trained stack's weights (learning=False)
"""

import os

import numpy as np

from . import _lib as L
from .engine import words_to_bool
from .group import ModelGroup, SharedStream
from .networks import HierarchicalTemporalMemory, _BatchedCall, _batches, _cached_bank, _check_encoder, _record_fields, retire_states
from .stack import CHUNK_STEPS, RegionStack, _check_shape

BUFFER_BYTES = 256 << 20        # the most the per-level buffers of all members hold in a chunk of run() (GroupStack.buffer_bytes)


def _align4(words):
    """`words` 32-bit words rounded up to 16 bytes: the members' parts of one buffer stay 16-byte aligned."""
    return (int(words) + 3) // 4 * 4


class GroupStack:
    """B RegionStacks of one shape stepped together (see the module's docstring).  `streams`: B; `levels`, `strides`, `links`: as
    RegionStack takes them; `seeds`: one per member (default 0 .. B-1) -- member b equals RegionStack(input_dim, levels, strides,
    seed=seeds[b], links=links) made at the same point of NumPy's global stream (a model draws its Spatial Pooler's permanences from
    it when it is made; set_permanence() sets them explicitly).  All members enqueue on ONE stream."""

    def __init__(self, streams, input_dim, levels, strides=None, seeds=None, device=0, links=None):
        B = int(streams)
        if B < 1:
            raise ValueError(f"streams must be at least 1 (got {streams})")
        seeds = list(range(B)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != B:
            raise ValueError(f"seeds: {B} values, got {len(seeds)}")
        levels, links = _check_shape(input_dim, levels, strides, links)
        stream = SharedStream(device)
        members = []
        for seed in seeds:
            models, below = [], int(input_dim)
            for i, lv in enumerate(levels):
                models.append(HierarchicalTemporalMemory(below, lv[0], lv[1], active_columns=lv[2] if len(lv) == 3 else None, seed=seed + i,
                                                         device=device, stream=stream))
                below = lv[0]
            members.append(RegionStack.of(models, links=links))
        self._setup(members)

    @classmethod
    def of(cls, stacks):
        """A GroupStack over B existing RegionStacks of equal shapes, links and stack step counts whose levels all enqueue on one
        stream (ValueError otherwise).  The stacks stay ordinary RegionStacks: after any GroupStack call each is as if it had made
        the call itself, and its own process() / run() continue from there."""
        stacks = list(stacks)
        if not stacks:
            raise ValueError("a group stack needs at least one member")
        for b, s in enumerate(stacks):
            if not isinstance(s, RegionStack):
                raise ValueError(f"member {b} is a {type(s).__name__}, not a RegionStack")
            if any(stacks[j] is s for j in range(b)):
                raise ValueError(f"member {b} is a member again")
        s0 = stacks[0]
        for b, s in enumerate(stacks):
            if len(s) != len(s0) or s.links != s0.links:
                raise ValueError(f"member {b}: {len(s)} levels with the links {s.links}, member 0 has {len(s0)} with {s0.links}")
            if s.steps != s0.steps:
                raise ValueError(f"member {b} has taken {s.steps} steps, member 0 {s0.steps}: the members' windows must stand alike")
        self = cls.__new__(cls)
        self._setup(stacks)
        return self

    @classmethod
    def views(cls, stack, n, fork=False):
        """n streams over ONE copy of a trained RegionStack's weights: level l is ModelGroup.views(stack.levels[l], n, fork).  The
        streams step with learning=False only (the default here; True is a ValueError); every stream's link state starts at 0."""
        if not isinstance(stack, RegionStack):
            raise ValueError(f"GroupStack.views: a RegionStack, got a {type(stack).__name__}")
        if int(n) < 1:
            raise ValueError("GroupStack.views: n must be at least 1")
        if stack.steps % stack._S:
            raise ValueError(f"GroupStack.views: the stack has taken {stack.steps} steps, not a multiple of {stack._S} (the product of the strides)")
        groups = [ModelGroup.views(m, int(n), fork) for m in stack.levels]
        members = []
        for b in range(int(n)):
            member = RegionStack.__new__(RegionStack)       # (RegionStack.of refuses views: a member here is the holder of its stream's state)
            member._setup([g.models[b] for g in groups], list(stack.links))
            members.append(member)
        self = cls.__new__(cls)
        self._setup(members, groups)
        return self

    def _setup(self, members, groups=None):
        s0 = members[0]
        self.members = members                      # member b's RegionStack: its levels, link states and step counter
        self.links, self.strides, self._period, self._S = s0.links, s0.strides, s0._period, s0._S
        # level l of every member as one group (ValueError where the shapes differ)
        self.groups = groups if groups is not None else [ModelGroup([s.levels[l] for s in members]) for l in range(len(s0))]
        e0 = s0.levels[0].engine
        stream = e0.stream_handle()
        for b, s in enumerate(members):
            for l, m in enumerate(s.levels):
                if m.engine.stream_handle() != stream or m.engine.device != e0.device:
                    raise ValueError(f"member {b}, level {l} enqueues on another stream than member 0's level 0: create every level of every "
                                     "member on one stream (HierarchicalTemporalMemory(stream=...))")
        self._steps = s0.steps
        self.chunk_steps = int(os.environ.get("BITHTM_STACK_CHUNK", CHUNK_STEPS))
        self.buffer_bytes = BUFFER_BYTES            # run(): the most the per-level buffers of all members hold (fewer bytes: shorter chunks)
        self.pool_scratch_bytes = L.POOL_SCRATCH_BYTES      # run(): the most scratch a pooling link's calls get (fewer bytes: more batches)
        self.lib = L.load()
        self._bufs = {}                             # run(): device buffers {(level, name): (address, 32-bit words)}, the members' parts in a row
        self.last_run_chunks = []                   # run(), diagnostic: the level-0 steps of each chunk

    def __len__(self):
        return len(self.members)

    def __del__(self):
        bufs, self._bufs = getattr(self, "_bufs", {}), {}
        if bufs:
            for g in getattr(self, "groups", []):
                for m in g.models:
                    if m.engine is not None and m.engine.h:
                        m.engine.sync()
            for ptr, _ in bufs.values():
                self.lib.hipFree(ptr)

    @property
    def steps(self):
        """Inputs every member has processed through this GroupStack or before it was adopted."""
        return self._steps

    @property
    def levels(self):
        """The ModelGroups, bottom first."""
        return self.groups

    def link_state(self, l, b):
        """(persistence uint8[C], prev bool[C]) of member b's pooling link between the levels l and l + 1 (copies)."""
        return self.members[b].link_state(l)

    def _check_members(self):
        for b, s in enumerate(self.members):
            if s.steps != self._steps:
                raise ValueError(f"member {b} has taken {s.steps} steps, the group stack {self._steps}: a member was stepped alone; "
                                 "make a new GroupStack.of() the stacks once they stand alike")
            s._check_levels()

    def _learning(self, learning):
        return self.groups[0]._learning(learning)

    # ---- the stepwise loop through the host
    def process(self, X, learning=None):
        """One input of every member, member b on X[b] (bool [B, input_dim]): level 0's group steps, and every upper level's whose
        window this step completes.  Returns a list with one entry per level: ModelGroup.process's RunRecord for the levels that
        stepped, None for those in the middle of a window.  The links go through the host (bithtm_amd/pooling.py per member): the
        convenience path and the yardstick of run()."""
        learning = self._learning(learning)
        B = len(self.members)
        X = np.asarray(X, dtype=np.bool_)
        e0 = self.groups[0].models[0].engine
        if X.shape != (B, e0.input_dim):
            raise ValueError(f"X: bool [{B}, {e0.input_dim}], got {X.shape}")
        self._check_members()
        out = [None] * len(self.groups)
        x = X
        for l, g in enumerate(self.groups):
            out[l] = g.process(x, learning=learning)
            if l + 1 == len(self.groups):
                break
            for s, m in zip(self.members, g.models):
                active = m.engine.read(L.F_ACTIVE_COLUMN, np.int32, m.engine.active_columns)
                pool = s._pool.get(l)
                if pool is not None:
                    pool.step(active, words_to_bool(m.engine.read(L.F_CELL_PREDICTION, np.uint32, m.engine.cell_words), m.cell_dim).any(axis=1))
                else:
                    s._window[l][active] = True
            if (self._steps + 1) % self._period[l + 1]:
                break
            x = np.stack([s._window[l].copy() if l not in s._pool else s._pool[l].row() for s in self.members])
            for s in self.members:
                s._window[l][:] = False
        self._steps += 1
        for s in self.members:
            s._steps += 1
        return out

    compute = process

    def reset(self, members=None):
        """A sequence reset of every level of the members flagged in `members` (bool [B]; None: all), one launch per level
        (ModelGroup.reset), and those members' link states cleared.  Only between windows (ValueError otherwise)."""
        if self._steps % self._S:
            raise ValueError(f"reset(): the stack has taken {self._steps} steps, not a multiple of {self._S} (the product of the "
                             "strides): an upper level is in the middle of a window")
        mask = self.groups[0]._member_mask(members, "members")
        self._check_members()
        for g in self.groups:
            g.reset(mask)
        for b, s in enumerate(self.members):
            if mask is None or mask[b]:
                for pool in s._pool.values():
                    pool.reset()

    # ---- the device path
    def _buffer(self, level, name, words):
        """Device address of the stack's buffer (level, name) of at least `words` 32-bit words (kept, made anew when too small)."""
        return self.groups[0].models[0].engine.kept_buffer(self._bufs, (level, name), words)

    def _chunk(self, steps, fields):
        """Level-0 steps per chunk: the largest multiple of the strides' product that is at most chunk_steps (and `steps`) and keeps
        what the members' per-level buffers hold per chunk within buffer_bytes; at least one window of the top level."""
        S, period, B = self._S, self._period, len(self.members)
        per_step = 0.0                              # bytes of chunk-sized buffers per level-0 step, all members
        for l, g in enumerate(self.groups):
            eng = g.models[0].engine
            shapes, words = eng.record_shapes(), 0
            if l + 1 < len(self.groups):
                if not (fields and "active_column" in fields):
                    words += shapes["active_column"][0]
                if l in self.members[0]._pool and not (fields and "column_prediction" in fields):
                    words += shapes["column_prediction"][0]
            if l > 0:
                words += eng.words
            per_step += 4.0 * B * words / period[l]
        fit = int(self.buffer_bytes // per_step) if per_step else steps
        return max(S, min(max(self.chunk_steps, 1), max(steps, 1), max(fit, 1)) // S * S)

    def run(self, inputs, steps, learning=None, use_graph=True, record=None, resets=None):
        """`steps` inputs of every member, member b from the rows of inputs[b] (bool [B, n_inputs, input_dim]), cycled, through all
        levels on the device: RegionStack.run's loop per chunk with every step of every level covering all members -- level 0's
        group runs recorded into stack-owned buffers, ONE htm_group_pack_columns / htm_group_pool_columns call fills the members'
        chunk banks of the next level, whose group runs over them, and so on; one stream, no host wait inside a chunk, one
        synchronisation at the end of the call.  Member b ends as RegionStack.run(inputs[b], steps) leaves its twin.
        `steps` and the steps taken so far must be multiples of the product of the strides (ValueError).  learning=None: True, or
        False over views (which refuse True).  `record`: as RegionStack.run; the call then returns records[b][l], member b's
        RunRecord of level l.  `resets`: not available (group runs take no resets)."""
        if resets is not None:
            raise NotImplementedError("sequence resets inside a group run are not available yet (the follow-up: k_tm_reset per "
                                      "member inside the group's launches); reset members with model.reset() between group calls")
        learning = self._learning(learning)
        S, nl, B = self._S, len(self.groups), len(self.members)
        steps = int(steps)
        if steps < 0 or steps % S or self._steps % S:
            raise ValueError(f"run(): steps ({steps}) and the steps taken so far ({self._steps}) must be multiples of {S}, the product "
                             "of the strides")
        fields = None if record is None else _record_fields(record)
        _check_encoder(None, fields, 0, 0)          # (a stack takes no encoder: "predicted_value" is a ValueError)
        g0 = self.groups[0]
        input_dim = g0.models[0].engine.input_dim
        inputs = np.asarray(inputs, dtype=np.bool_)
        if inputs.ndim != 3 or inputs.shape[0] != B or inputs.shape[1] < 1 or inputs.shape[2] != input_dim:
            raise ValueError(f"inputs: bool [{B}, n_inputs, {input_dim}], got {inputs.shape}")
        self._check_members()
        n_rows = inputs.shape[1]
        for g in self.groups:
            for m in g.models:
                retire_states(m.engine)
        period = self._period
        chunk = self._chunk(steps, fields)
        shapes = [g.models[0].engine.record_shapes() for g in self.groups]
        ks = [g.models[0].active_columns for g in self.groups]
        pooled = self.members[0]._pool
        # what each level records, per member: the user's fields over the whole call (read back at its end), and, below another
        # level, its active columns (and under a pooling link its column prediction) -- over one chunk if the user did not ask
        rows = []
        for l in range(nl):
            want = dict.fromkeys(fields or (), steps // period[l])
            if l + 1 < nl:
                want.setdefault("active_column", chunk // period[l])
                if l in pooled:
                    want.setdefault("column_prediction", chunk // period[l])
            rows.append(want)
        pools = {l: self._pool_buffers(l, chunk // period[l + 1]) for l in pooled if steps}
        self.last_run_chunks = []
        engines0 = [m.engine for m in g0.models]
        banks = [_cached_bank(m, m.engine, x) for m, x in zip(g0.models, inputs)]
        call = _BatchedCall([m.temporal_memory for s in self.members for m in s.levels], fields)

        def segment_pools():                        # default-sized pools grow as in group runs: a look between chunks, all members alike
            nonlocal banks, engines0
            for l, g in enumerate(self.groups):
                if not g._auto_grow:
                    continue
                while g._grow(2 * ks[l], True):
                    pass
                yield min(m.engine._free_segments for m in g.models), 2 * ks[l], period[l]
            if any(m.engine is not e for m, e in zip(g0.models, engines0)):     # (level 0's banks on its new engines)
                engines0 = [m.engine for m in g0.models]
                banks = [_cached_bank(m, m.engine, x, fresh=True) for m, x in zip(g0.models, inputs)]
        for done, n in _batches(steps, segment_pools, cap=chunk, multiple=S):
            below = below_pred = None               # per member: device addresses of the lists (and column predictions) of the level below
            for l, g in enumerate(self.groups):
                n_l, done_l = n // period[l], done // period[l]
                bufs = [{} for _ in range(B)]
                for f, total in rows[l].items():
                    w = shapes[l][f][0]
                    whole = fields is not None and f in fields
                    part = _align4(max(total, 1) * w)
                    base = self._buffer(l, f, B * part) + (4 * done_l * w if whole else 0)
                    for b in range(B):
                        bufs[b][f] = base + 4 * b * part
                if l == 0:
                    level_banks, bank_rows = banks, n_rows
                else:
                    # (a run reads bank row step_index % n_inputs of ITS handle: a member's rows of the chunk start at that row)
                    words = g.models[0].engine.words
                    part = (chunk // period[l]) * words
                    base = self._buffer(l, "bank", B * part)
                    level_banks, bank_rows = [base + 4 * b * part for b in range(B)], n_l
                    first_rows = [m.engine.steps % n_l for m in g.models]
                    if l - 1 in pools:
                        persistence, prev, scratch, scratch_bytes = pools[l - 1]
                        g.pool_columns(self.links[l - 1], below, ks[l - 1], below_pred, n_l, persistence, prev, None, scratch, scratch_bytes,
                                       level_banks, n_l, first_rows)
                    else:
                        g.pack_columns(below, ks[l - 1], n_l, self.strides[l - 1], level_banks, n_l, first_rows)
                g.run_into(level_banks, bank_rows, n_l, bufs, learning=learning, use_graph=use_graph)
                below, below_pred = [b.get("active_column") for b in bufs], [b.get("column_prediction") for b in bufs]
            self._steps += n
            for s in self.members:
                s._steps += n
            self.last_run_chunks.append(n)
        e0 = g0.models[0].engine
        totals = [steps // p for p in period]
        if pools:                                   # the links' states come home behind the call's one wait
            e0.sync()
            for l, (persistence, prev, _, _) in pools.items():
                C = self.members[0]._pool[l].column_dim
                for b, s in enumerate(self.members):
                    s._pool[l].persistence[:] = e0.read_words(persistence[b], (C + 3) // 4, np.uint32).view(np.uint8)[:C]
                    s._pool[l].prev[:] = np.unpackbits(e0.read_words(prev[b], (C + 31) // 32, np.uint32).view(np.uint8), bitorder="little")[:C]

        def read():                                 # (after finish() has synchronised: an overflow is reported by the call it happened in)
            out = []
            for b in range(B):
                for l, n in enumerate(totals):
                    part = {}
                    for f in fields:
                        w, dtype = shapes[l][f]
                        address = self._bufs[(l, f)][0] + 4 * b * _align4(max(n, 1) * w)
                        part[f] = e0.read_words(address, n * w, dtype).reshape(n, w)
                    out.append(part)
            return out
        records = call.finish(totals * B, ks * B, read=read)
        return None if fields is None else [records[b * nl:(b + 1) * nl] for b in range(B)]

    def _pool_buffers(self, l, windows):
        """The device side of the pooling link l for a run() whose chunks hold at most `windows` of its windows: (each member's
        persistence, each member's prev, scratch, scratch bytes), the state arrays holding the members' host states.  Called before
        the call's first launch: the stream is at rest (every run() ends with a wait), so the copies order themselves."""
        B = len(self.members)
        pool0, upper = self.members[0]._pool[l], self.groups[l + 1].models[0]
        C = pool0.column_dim
        if C > L.POOL_MAX_COLUMNS:
            raise ValueError(f"link {l}: a pooling link serves at most {L.POOL_MAX_COLUMNS} lower columns on the device (level {l} has {C})")
        window = (pool0.link.stride + 8) * 4 * upper.engine.words          # (htm_group_pool_columns: a window's bitmap rows and its snapshot row, per member)
        if B * window > self.pool_scratch_bytes:
            raise ValueError(f"link {l}: one window of {B} members needs {B * window} bytes of scratch, above the bound of {self.pool_scratch_bytes} "
                             "(pool_scratch_bytes)")
        scratch_bytes = min(self.pool_scratch_bytes // (B * window), max(windows, 1)) * B * window
        p_words, v_words = _align4((C + 3) // 4), _align4((C + 31) // 32)
        p_base = self._buffer(l, "pool_persistence", B * p_words)
        v_base = self._buffer(l, "pool_prev", B * v_words)
        scratch = self._buffer(l, "pool_scratch", (scratch_bytes + 3) // 4)
        eng = upper.engine
        P = np.zeros((B, 4 * p_words), dtype=np.uint8)
        V = np.zeros((B, 4 * v_words), dtype=np.uint8)
        for b, s in enumerate(self.members):
            P[b, :C] = s._pool[l].persistence
            bits = np.packbits(s._pool[l].prev, bitorder="little")
            V[b, :bits.size] = bits
        for ptr, data in ((p_base, P), (v_base, V)):
            eng._hip_check(self.lib.hipMemcpy(ptr, data.ctypes.data, data.nbytes, L.HIP_MEMCPY_HOST_TO_DEVICE), "hipMemcpy")
        return [p_base + 4 * b * p_words for b in range(B)], [v_base + 4 * b * v_words for b in range(B)], scratch, scratch_bytes

    # ---- checkpoints
    def state_dict(self):
        """A list of B dictionaries in RegionStack.state_dict's format: a RegionStack of the same shape loads member b's."""
        return [s.state_dict() for s in self.members]

    def load_state_dict(self, states):
        """ValueError for another number of members, for a member's dictionary of another shape (RegionStack.load_state_dict), or
        for dictionaries whose stack step counts differ."""
        states = list(states)
        if len(states) != len(self.members):
            raise ValueError(f"load_state_dict(): {len(self.members)} dictionaries, one per member, got {len(states)}")
        counts = {int(st["stack_steps"]) if "stack_steps" in st else None for st in states}
        if len(counts) != 1 or None in counts:
            raise ValueError(f"load_state_dict(): the members' stack step counts differ or are missing ({sorted(counts, key=str)})")
        for s, st in zip(self.members, states):
            s.load_state_dict(st)
        self._steps = counts.pop()
