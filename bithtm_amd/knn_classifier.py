"""KNNClassifier: NuPIC's KNN classifier over active-cell patterns, kept on the device (htm_knn_*, include/bithtm_hip.h; DESIGN.md
section 26).  The definition is knn.py; the device equals it bit for bit.

    knn = KNNClassifier(labels=12, k=3, capacity=16384)              # bound to a device, and to a model's shape, at first use
    model.run(inputs, 600, knn=knn, labels=names)                   # names int [rows of inputs], -1: no label: the labelled steps are stored
    rec = view.run(inputs, 200, knn=knn)                            # rec.knn_label, knn_votes, knn_overlap, knn_nearest_slot, knn_nearest_step
    best, votes = knn.update_patterns(index, words, labels)         # the stand-alone door: patterns as (word index, word) pairs

Memory: capacity x (8 max_pairs + 12) bytes of store and 128 x capacity bytes of overlaps -- 7.6 MiB at 16 384 slots of 40 pairs."""

import ctypes as C
import weakref

import numpy as np

from . import _lib as L
from .classifier import check_patterns
from .engine import HtmError
from .knn import MAX_PAIRS, check_params, is_label
from .sdr_classifier import model_shape


class _DeviceKNN:
    """`streams` KNN classifier streams of one config in one device object: the parameters, the shape of the patterns, the lazy binding
    to a device, the device object's life, and every call, written once over a leading stream axis -- labels [streams, n], patterns
    [streams, T, n], best [streams, n, 5], votes [streams, n, labels], counts int64 [streams], a state whose stores lie one behind the
    other in stream order.  KNNClassifierBank is this with its own axis; KNNClassifier is the one stream whose arguments and results
    come without the axis (_lift puts it on, _drop takes it off) and whose calls go through the one-stream C functions.  Neither is an
    instance of the other."""

    _prefix = None                              # of the C functions the calls go through: htm_knn_ or htm_knns_
    _what = None
    _single = False                             # the public arrays come without the stream axis
    streams = 1
    source = None                               # KNNClassifierBank.shared(): the KNNClassifier whose store the streams read

    def _init(self, labels, k, min_overlap, capacity, shape):
        self.labels, self.k, self.min_overlap, self.capacity = check_params(labels, k, min_overlap, capacity)
        self.shape = None
        if shape is not None:
            self._set_shape(*shape)
        self.lib = None
        self.device = None
        self._knn = None
        self._last = None                       # weak reference to the engine of the last call
        self._home = None                       # a small model of the object's own, made when no other handle is there
        self._bufs = {}                         # the device buffers of a call's outputs: name -> (address, words)
        self._pending = None                    # a state loaded before the object was bound
        self._counts, self._total = np.zeros(self.streams, dtype=np.int64), 0       # the host's mirror: nothing is read back to know them

    def _create(self, engine, cfg, out):
        raise NotImplementedError

    def _pointers(self, a):
        """A call's device addresses of its pairs -- one, or a sequence of `streams` -- as the update's C function takes them."""
        return C.c_void_p(a) if self._single else (C.c_void_p * self.streams)(*[int(x) for x in a])

    def _no_shared_learning(self, learning):
        pass                                    # (KNNClassifierBank.shared() refuses here)

    @property
    def _axis(self):
        """The stream axis in the shapes of the public arrays: (streams,), or nothing for the one stream."""
        return () if self._single else (self.streams,)

    def _lift(self, a):
        return a[None] if self._single else a

    def _drop(self, a):
        return a[0] if self._single else a

    def _dims(self, *tail):
        return "[" + ", ".join(str(x) for x in self._axis + tail) + "]"

    def _set_shape(self, column_dim, cell_dim, max_pairs):
        column_dim, cell_dim, max_pairs = int(column_dim), int(cell_dim), int(max_pairs)
        if column_dim < 1 or not 1 <= cell_dim <= 64 or not 1 <= max_pairs <= MAX_PAIRS:
            raise ValueError(f"{self._what}: shape = (column_dim >= 1, cell_dim in [1, 64], max_pairs in [1, {MAX_PAIRS}]), got "
                             f"{(column_dim, cell_dim, max_pairs)}")
        shape = (column_dim, cell_dim, max_pairs)
        if self.shape is not None and self.shape != shape:
            raise ValueError(f"the KNN classifier was made for patterns of shape {self.shape} (column_dim, cell_dim, pairs), this call has {shape}")
        self.shape = shape

    @property
    def units(self):
        return self.shape[0] * self.shape[1]

    @property
    def total(self):
        """Steps seen."""
        return int(self._pending["total"]) if self._knn is None and self._pending is not None else self._total

    @property
    def count(self):
        """Slots in use: per stream, int64 [streams] (shared(): zeros -- the store is the owner's); KNNClassifier: an int."""
        counts = self._pending["count"] if self._knn is None and self._pending is not None else self._counts
        return int(counts[0]) if self._single else np.array(counts, dtype=np.int64)

    # ---- binding
    def _bind(self, engine):
        if self.shape is None:
            raise RuntimeError(f"the KNN classifier does not know the shape of its patterns yet: use it with a model, or give {self._what}(shape=)")
        if self._knn is None:
            self.lib = engine.lib
            cfg = L.HtmKnnConfig(C.sizeof(L.HtmKnnConfig), self.labels, self.k, self.min_overlap, self.capacity, self.units, self.shape[1], self.shape[2])
            out = C.c_void_p()
            rc = self._create(engine, cfg, out)
            if rc != 0:
                raise HtmError(f"{self._prefix}create failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")
            self._knn, self.device = out, engine.device
            self._last = weakref.ref(engine)
            if self._pending is not None:
                pending, self._pending = self._pending, None
                self._import(engine, pending)
        elif engine.device != self.device:
            raise ValueError(f"the KNN classifier lives on device {self.device}, the model on device {engine.device}")
        # the library orders calls on one stream only: what the last engine enqueued is waited for before another engine touches the state
        last = self._last() if self._last is not None else None
        if last is not None and last is not engine and getattr(last, "h", None):
            last.sync()
        self._last = weakref.ref(engine)
        return engine

    def bind(self, model):
        """Bind the object to `model`'s device now -- and, unless it was given one, to the shape of the model's patterns.  Returns
        the object."""
        if self.shape is None:
            self._set_shape(*model_shape(model.engine))
        self._bind(model.engine)
        return self

    def _engine(self, device=None):
        engine = self._last() if self._last is not None else None
        if engine is not None and getattr(engine, "h", None) and device in (None, engine.device):
            return self._bind(engine)
        if self._knn is not None and device not in (None, self.device):
            raise ValueError(f"the KNN classifier lives on device {self.device}, not {device}")
        if self._home is None:
            if device is None and self.device is None:
                raise RuntimeError("the KNN classifier is not bound to a device yet: use it with a model, or give update_patterns(device=)")
            from .networks import HierarchicalTemporalMemory
            self._home = HierarchicalTemporalMemory(32, 64, 4, active_columns=4, device=self.device if device is None else int(device))
        return self._bind(self._home.engine)

    def __del__(self):
        knn, self._knn = getattr(self, "_knn", None), None
        if knn:
            self.lib.htm_knn_destroy(knn)
        for ptr, _ in getattr(self, "_bufs", {}).values():
            self.lib.hipFree(ptr)

    def _call(self, engine, name, *args):
        what = self._prefix + name
        rc = getattr(self.lib, what)(self._knn, engine.h, *args)
        if rc < 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")

    # ---- what a call stores, decided here
    def check_labels(self, labels):
        """int [streams, n] -> int32: any value outside [0, labels) is no label (-1)."""
        g = np.asarray(labels)
        if g.ndim != len(self._axis) + 1 or self._lift(g).shape[0] != self.streams or g.dtype.kind not in "iu":
            raise ValueError(f"labels: int {self._dims('n')}, got {g.dtype} {list(g.shape)}")
        g = g.astype(np.int64)
        return np.ascontiguousarray(np.where((g < 0) | (g >= self.labels), -1, g).astype(np.int32))

    def stored_by(self, labels, first_step, n, learning):
        """int64 [streams] (KNNClassifier: an int): the patterns a call of n steps would store per stream; step i reads
        labels[s][(first_step + i) % rows]."""
        stored = np.zeros(self.streams, dtype=np.int64)
        if learning and n > 0:
            flags = self._lift(np.asarray(labels)) >= 0
            rows = flags.shape[1]
            whole, rest = divmod(int(n), rows)
            at = (int(first_step) + np.arange(rest)) % rows
            stored = (whole * flags.sum(axis=1) + flags[:, at].sum(axis=1)).astype(np.int64)
        return int(stored[0]) if self._single else stored

    def check_room(self, stored):
        """ValueError for a call that would take ANY stream past capacity: refused as a whole before anything is enqueued."""
        stored, count = self._lift(np.asarray(stored)), self._lift(np.asarray(self.count))
        over = np.nonzero(count + stored > self.capacity)[0]
        if over.size:
            i = int(over[0])
            raise ValueError(f"knn: {'' if self._single else f'stream {i}: '}the call would store {int(stored[i])} patterns in a store of {int(count[i])} "
                             f"of capacity = {self.capacity} slots")

    def upload_labels(self, engine, labels):
        """int32 [streams, n] (check_labels) -> the device address of the labels of a run's rows (the object's own array: the C labels
        call)."""
        self._bind(engine)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        out = C.c_void_p()
        self._call(engine, "labels", labels.ctypes.data_as(C.c_void_p), self._lift(labels).shape[1], C.byref(out))
        return out.value

    # ---- the update over device memory (what run() and ModelGroup.run() call; nothing here waits)
    def pairs_buffer(self, engine, n):
        """The device address of a buffer [streams][n][max_pairs] pairs (kept)."""
        self._bind(engine)
        return engine.kept_buffer(self._bufs, "pairs", 2 * self.streams * max(int(n), 1) * self.shape[2], spare=2)

    def enqueue(self, engine, device_pairs, pairs_per_step, n, device_labels, host_labels, first_step, learning, votes=False):
        """ONE update of every stream over n steps' patterns in device memory (device_pairs: `streams` addresses; KNNClassifier: one),
        enqueued on `engine`'s stream; device_labels is upload_labels' address of host_labels (int32 [streams, rows]; a bank takes
        None for both in a frozen call).  read(engine, n, votes) after the stream's wait gives the results.  ValueError, with
        nothing enqueued, for a call in which any stream does not fit its store."""
        self._bind(engine)
        n, S = int(n), self.streams
        self._no_shared_learning(learning)
        stored = self.stored_by(host_labels, first_step, n, learning and host_labels is not None)
        self.check_room(stored)
        rows = self._lift(host_labels).shape[1] if host_labels is not None else 1
        best = engine.kept_buffer(self._bufs, "best", S * max(n, 1) * 5, spare=2)
        all_votes = engine.kept_buffer(self._bufs, "votes", S * max(n, 1) * self.labels, spare=2) if votes else None
        self._call(engine, "update", self._pointers(device_pairs), int(pairs_per_step), n, C.c_void_p(device_labels) if device_labels else None, rows,
                   int(first_step), int(bool(learning)), C.c_void_p(best), C.c_void_p(all_votes) if all_votes else None)
        self._counts += stored
        self._total += n

    def read(self, engine, n, votes=False):
        """(best int32 [streams, n, 5], votes int32 [streams, n, labels] or None) of the last enqueue, after the engine's stream has
        been waited for."""
        n, S = int(n), self.streams
        best = engine.read_words(self._bufs["best"][0], S * n * 5, np.int32).reshape(S, n, 5)
        all_votes = engine.read_words(self._bufs["votes"][0], S * n * self.labels, np.int32).reshape(S, n, self.labels) if votes else None
        return self._drop(best), (self._drop(all_votes) if votes else None)

    # ---- the stand-alone door
    def update_patterns(self, index, words, labels=None, learning=True, votes=False, device=None):
        """T further steps of every stream from their patterns: index int [S, T, n], words uint32 [S, T, n] (pair j of step t is
        (index[t, j], words[t, j]); a negative index or a zero word contributes nothing), labels int [S, T] (outside [0, labels):
        none; a bank's None: nothing is labelled).  Checked here: the indices of a step are distinct and inside the table, no word
        has a bit at or above cell_dim, n <= max_pairs, every stream's labelled steps fit its store -- a call in which any stream's
        do not is refused as a whole.  -> (best int32 [S, T, 5]: label, votes, nearest_overlap, nearest_slot, nearest_step; votes
        int32 [S, T, labels] or None)."""
        if self.shape is None:
            raise RuntimeError(f"the KNN classifier does not know the shape of its patterns yet: use it with a model, or give {self._what}(shape=)")
        S = self.streams
        if not self._single:
            index, words = np.asarray(index), np.asarray(words)
            if index.ndim != 3 or index.shape[0] != S or words.shape != index.shape:
                raise ValueError(f"patterns: index int [{S}, T, n] and words uint32 [{S}, T, n], got {index.shape} and {words.shape}")
            index, words = (a.reshape(S * a.shape[1], a.shape[2]) for a in (index, words))
        index, words = check_patterns(index, words, self.units, self.shape[1])              # (every stream's steps, one behind the other)
        T, n = index.shape[0] // S, index.shape[1]
        if not 1 <= n <= self.shape[2]:
            raise ValueError(f"patterns: 1 to max_pairs = {self.shape[2]} pairs per step, got {n}")
        labels = self._lift(self.check_labels(np.full((S, max(T, 1)), -1) if labels is None and not self._single else labels))
        if (T or self._single) and labels.shape != (S, T):
            raise ValueError(f"labels: int {self._dims(T)}, got {list(self._drop(labels).shape)}")
        learning = bool(learning)
        self._no_shared_learning(learning)
        self.check_room(self.stored_by(self._drop(labels), 0, T, learning))
        if T == 0:
            return self._drop(np.zeros((S, 0, 5), np.int32)), (self._drop(np.zeros((S, 0, self.labels), np.int32)) if votes else None)
        engine = self._engine(device)
        pairs = np.empty((S, T, n, 2), dtype=np.int32)
        pairs[..., 0], pairs[..., 1] = index.reshape(S, T, n), words.view(np.int32).reshape(S, T, n)
        buf = engine.device_buffer(pairs.nbytes, pairs)
        try:
            labelled = learning or self._single             # (the one stream always passes its labels)
            device_labels = self.upload_labels(engine, self._drop(labels)) if labelled else None
            self.enqueue(engine, self._drop([buf + i * T * n * 8 for i in range(S)]), n, T, device_labels, self._drop(labels) if labelled else None, 0, learning,
                         votes)
            engine.sync()
            best, all_votes = self.read(engine, T, votes)
            return best.copy(), (all_votes.copy() if votes else None)
        finally:
            engine.sync()
            self.lib.hipFree(buf)

    # ---- reset, state: kept with the stream axis (count int64 [streams], the stores one behind the other), also while pending
    def _reset(self, flags):
        """Empty every stream's store, or those `flags` (uint8 [streams]) names."""
        if self._knn is None:
            if self._pending is not None:
                keep = np.zeros(self.streams, bool) if flags is None else flags == 0
                self._pending = self._select(self._pending, keep)
            return
        self._call(self._engine(), "reset", *(() if self._single else (flags.ctypes.data_as(C.c_void_p) if flags is not None else None,)))
        self._counts = np.where(flags == 0, self._counts, 0) if flags is not None else np.zeros(self.streams, dtype=np.int64)

    def _select(self, state, keep):
        """`state` with the stores of the streams not in `keep` (bool [streams]) emptied."""
        counts = np.asarray(state["count"], dtype=np.int64)
        rows = np.repeat(keep, counts)
        return dict(total=state["total"], count=np.where(keep, counts, 0), pairs=state["pairs"][rows], labels=state["labels"][rows], stamps=state["stamps"][rows])

    def _empty_state(self):
        pairs = np.zeros((0, self.shape[2], 2), dtype=np.int32)
        return dict(total=np.int64(0), count=np.zeros(self.streams, np.int64), pairs=pairs, labels=np.zeros(0, np.int32), stamps=np.zeros(0, np.int64))

    def _params(self):
        return (self.labels, self.k, self.min_overlap, self.capacity) + (self.shape or ())

    def state_dict(self):
        """{"params": int64 [labels, k, min_overlap, capacity, column_dim, cell_dim, max_pairs], "streams": int64, "total": int64,
        "count": int64 [streams], "pairs": int32 [sum of count, max_pairs, 2], "labels": int32 [sum], "stamps": int64 [sum]} -- the
        streams' stores one behind the other in stream order, read from the device (shared(): counts 0 -- the store is the owner's;
        KNNClassifier: "count" one int64 and no "streams")."""
        if self.shape is None:
            raise RuntimeError("the KNN classifier does not know the shape of its patterns yet")
        if self._knn is None:
            state = self._pending if self._pending is not None else self._empty_state()
        else:
            engine = self._engine()
            S, n, P = self.streams, int(self._counts.sum()), self.shape[2]
            head = 8 * (1 + S)
            size = head + n * (8 * P + 12)
            assert size == self.info()["state_bytes"]
            blob = np.zeros(size, dtype=np.uint8)
            self._call(engine, "export", blob.ctypes.data_as(C.c_void_p), size)
            words = blob[:head].view(np.int64)
            at = head + n * P * 8
            state = dict(total=np.int64(words[0]), count=words[1:], pairs=blob[head:at].view(np.int32).reshape(n, P, 2),
                         stamps=blob[at:at + n * 8].view(np.int64), labels=blob[at + n * 8:].view(np.int32))
        out = {k: np.array(self._drop(v) if k == "count" else v)[()] for k, v in state.items()}        # (copies; [()]: a scalar of a 0-d array)
        return dict(out, params=np.asarray(self._params(), dtype=np.int64), **({} if self._single else {"streams": np.int64(self.streams)}))

    def load_state_dict(self, state):
        """The state of a state_dict() of an object with the same parameters, shape and streams."""
        params = tuple(int(x) for x in state["params"])
        if self.shape is None and len(params) == 7:
            self._set_shape(*params[4:])
        streams = 1 if self._single else int(state["streams"])
        if params != self._params() or streams != self.streams:
            theirs, mine = ("", "") if self._single else (f" and {streams} streams", f" and {self.streams}")
            raise ValueError(f"the state was saved with parameters {params} (labels, k, min_overlap, capacity, column_dim, cell_dim, max_pairs){theirs}, "
                             f"this object has {self._params()}{mine}")
        total = int(state["total"])
        counts = np.ascontiguousarray(self._lift(np.asarray(int(state["count"]) if self._single else state["count"], dtype=np.int64)))
        pairs = np.ascontiguousarray(state["pairs"], dtype=np.int32)
        labels = np.ascontiguousarray(state["labels"], dtype=np.int32)
        stamps = np.ascontiguousarray(state["stamps"], dtype=np.int64)
        top = 0 if self.source is not None else self.capacity
        if counts.shape != (self.streams,) or (counts < 0).any() or (counts > top).any() or total < 0:
            if self._single:
                raise ValueError(f"state: 0 <= count <= capacity = {self.capacity} and total >= 0, got count {int(counts[0])}, total {total}")
            raise ValueError(f"state: count int64 [{self.streams}] with 0 <= count <= {top} and total >= 0, got count {counts.tolist()}, total {total}")
        n = int(counts.sum())
        for name, a, want in (("pairs", pairs, (n, self.shape[2], 2)), ("labels", labels, (n,)), ("stamps", stamps, (n,))):
            if a.shape != want:
                raise ValueError(f"state['{name}']: {list(want)}, got {list(a.shape)}")
        if n and (labels.min() < 0 or labels.max() >= self.labels):
            raise ValueError(f"state['labels']: a label outside [0, {self.labels})")
        at = 0
        for c in counts.tolist():
            mine = stamps[at:at + c]
            if c and (mine[0] < 0 or mine[-1] >= total or (np.diff(mine) <= 0).any()):
                whose = "the" if self._single else "every stream's"
                raise ValueError(f"state['stamps']: {whose} stamps ascend and lie below total")
            at += c
        clean = dict(total=np.int64(total), count=counts.copy(), pairs=pairs.copy(), labels=labels.copy(), stamps=stamps.copy())
        if self._knn is None:
            self._pending = clean
        else:
            self._import(self._engine(), clean)

    def _import(self, engine, state):
        head = np.concatenate([[int(state["total"])], np.asarray(state["count"], dtype=np.int64)]).astype(np.int64)
        blob = np.concatenate([head.view(np.uint8), state["pairs"].view(np.uint8).ravel(), state["stamps"].view(np.uint8).ravel(),
                               state["labels"].view(np.uint8).ravel()])
        self._call(engine, "import", blob.ctypes.data_as(C.c_void_p), blob.size)
        self._counts, self._total = np.asarray(state["count"], dtype=np.int64).copy(), int(state["total"])


class KNNClassifier(_DeviceKNN):
    """The classifier of `labels` labels: a step's result is the label most of its `k` nearest stored patterns carry, nearest by
    overlap (at least `min_overlap`), in a store of `capacity` slots that never overwrites.  The shape of the patterns --
    column_dim, cell_dim and the pairs a pattern has at most -- comes from the model of the first run(knn=), or from
    `shape=(column_dim, cell_dim, max_pairs)` for stand-alone use.  The object binds to a device lazily, as SDRClassifier does;
    every update continues where the last one ended, whichever door it came through.  The calls are _DeviceKNN's for one stream,
    without the stream axis: labels int [n], patterns [T, n], best [n, 5], votes [n, labels], `count` an int, a state of "count": int64
    and no "streams"."""

    _prefix = "htm_knn_"
    _what = "KNNClassifier"
    _single = True

    def __init__(self, labels, k=1, min_overlap=1, capacity=4096, shape=None):
        self._init(labels, k, min_overlap, capacity, shape)

    def _create(self, engine, cfg, out):
        return self.lib.htm_knn_create(engine.h, C.byref(cfg), C.byref(out))

    def info(self):
        """htm_knn_info of the bound object as a dict (the form of the distance launch among it)."""
        out = L.HtmKnnInfo(C.sizeof(L.HtmKnnInfo))
        if self._knn is None or self.lib.htm_knn_info(self._knn, C.byref(out)) != 0:
            raise RuntimeError("the KNN classifier is not bound to a device yet")
        return {name: int(getattr(out, name)) for name, _ in L.HtmKnnInfo._fields_[1:]}

    def update_patterns(self, index, words, labels, learning=True, votes=False, device=None):
        """T further steps from their patterns: index int [T, n], words uint32 [T, n], labels int [T] -> (best int32 [T, 5], votes int32
        [T, labels] or None), as _DeviceKNN.update_patterns describes them."""
        return super().update_patterns(index, words, labels, learning, votes, device)

    def reset(self):
        """Empty the store (count = 0; the step total stays)."""
        self._reset(None)


class KNNClassifierBank(_DeviceKNN):
    """`streams` independent KNNClassifier streams of one config in one device object (htm_knns_*): stream i fed
    (patterns_i, labels_i) equals a KNNClassifier fed the same, bit for bit, and every call steps all streams in the launches of
    one, whatever `streams` is.  The streams share one step total.

        bank = KNNClassifierBank(64, labels=12, k=3, capacity=4096, shape=(2048, 32, 40))
        best, votes = bank.update_patterns(index, words, labels)        # index, words [64, T, P], labels [64, T]
        group.run(inputs, 600, knn=bank, labels=names)                  # names int [64, rows of inputs]
        views = KNNClassifierBank.shared(knn, 4)                        # four frozen streams over knn's store, read where it lies

    Memory: streams x capacity x (8 max_pairs + 12) bytes of stores and the scratch info() reports; shared() holds scratch only."""

    _prefix = "htm_knns_"
    _what = "KNNClassifierBank"

    def __init__(self, streams, labels, k=1, min_overlap=1, capacity=4096, shape=None):
        self._init(labels, k, min_overlap, capacity, shape)
        self.streams = int(streams)
        if not 1 <= self.streams <= L.KNNS_MAX_STREAMS:
            raise ValueError(f"KNNClassifierBank: streams must be in [1, {L.KNNS_MAX_STREAMS}], got {streams}")
        self._counts = np.zeros(self.streams, dtype=np.int64)

    @classmethod
    def shared(cls, knn, streams):
        """A bank of `streams` frozen streams that infer over the store of `knn`, a bound KNNClassifier, as it is at each call: no
        copy, every slot in [0, knn.count) is seen -- what knn stores later the next call here sees.  The bank keeps a reference to
        knn; its own state is the step total.  Learning through the bank is refused."""
        if not isinstance(knn, KNNClassifier):
            raise ValueError("KNNClassifierBank.shared(): knn is a one-stream KNNClassifier")
        if knn._knn is None:
            raise ValueError("KNNClassifierBank.shared(): knn is not bound to a device yet (use it with a model, or knn.bind(model))")
        bank = cls(streams, knn.labels, knn.k, knn.min_overlap, knn.capacity, knn.shape)
        bank.source = knn
        bank._last = knn._last                  # (its calls go through the engine knn's last call came through, until a model brings its own)
        return bank

    def _create(self, engine, cfg, out):
        share = None
        if self.source is not None:
            if self.source._knn is None or self.source.device != engine.device:
                raise ValueError(f"the shared KNN classifier lives on device {self.source.device}, the model on device {engine.device}")
            share = self.source._knn
        return self.lib.htm_knns_create(engine.h, C.byref(cfg), self.streams, share, C.byref(out))

    def _bind(self, engine):
        if self.source is not None:             # (what the owner's last engine enqueued on the store is waited for first)
            owner = self.source._last() if self.source._last is not None else None
            if owner is not None and owner is not engine and getattr(owner, "h", None):
                owner.sync()
        return super()._bind(engine)

    def _no_shared_learning(self, learning):
        if learning and self.source is not None:
            raise ValueError("KNNClassifierBank.shared(): the streams read one store -- learning is refused (the owner stores through its own calls)")

    def info(self):
        """htm_knns_info of the bound object as a dict (the chunk and the scratch and device bytes among it)."""
        out = L.HtmKnnsInfo(C.sizeof(L.HtmKnnsInfo))
        if self._knn is None or self.lib.htm_knns_info(self._knn, C.byref(out), None) != 0:
            raise RuntimeError("the KNN classifier bank is not bound to a device yet")
        return {name: int(getattr(out, name)) for name, _ in L.HtmKnnsInfo._fields_[1:] if name != "reserved"}

    def reset(self, streams=None):
        """Empty every stream's store, or those `streams` (bool [streams]) names (the total stays)."""
        flags = None
        if streams is not None:
            flags = np.ascontiguousarray(np.asarray(streams, dtype=np.bool_).ravel()).astype(np.uint8)
            if flags.shape != (self.streams,):
                raise ValueError(f"streams: bool [{self.streams}], got {list(flags.shape)}")
        self._reset(flags)

    def stream_state(self, i):
        """Stream i's state as a one-stream KNNClassifier of the same parameters loads it (load_state_dict)."""
        i = int(i)
        if not 0 <= i < self.streams:
            raise ValueError(f"stream: in [0, {self.streams}), got {i}")
        state = self.state_dict()
        lo = int(state["count"][:i].sum())
        hi = lo + int(state["count"][i])
        return dict(params=state["params"], total=state["total"], count=np.int64(hi - lo), pairs=state["pairs"][lo:hi].copy(),
                    labels=state["labels"][lo:hi].copy(), stamps=state["stamps"][lo:hi].copy())
