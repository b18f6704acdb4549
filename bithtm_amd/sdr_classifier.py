"""SDRClassifier: NuPIC's SDR classifier kept on the device (htm_classifier_*, include/bithtm_hip.h).  The
definition is classifier.py; the device equals it bit for bit.

    enc = ScalarEncoder([ScalarField(0, 100, 64, 9)])
    clf = SDRClassifier(field=enc.fields[0], steps=(1, 5))          # bound to a device, and to a model's shape, at first use
    rec = model.run(values, 5000, encoder=enc, classifier=clf)      # rec.classified_bucket [steps, 2], _probability, _value
    best, dist = clf.update_patterns(index, words, targets)         # the stand-alone door: patterns as (word index, word) pairs

Memory: units x B_pad x 4 bytes per horizon (units = column_dim * cell_dim, B_pad = buckets rounded up to 4) -- 32 MiB at 2 048 columns
of 32 cells with 128 buckets, 1 GiB at 65 536 columns."""

import ctypes as C
import weakref

import numpy as np

from . import _lib as L
from .classifier import EXP_TABLE, W_LIMIT, check_params, check_patterns
from .encoders import FIELD_COORDINATE
from .engine import HtmError


class _DeviceClassifier:
    """`streams` classifier streams of one config in one device object: the parameters, the shape of the patterns, the lazy binding to
    a device (as AnomalyLikelihood binds), the device object's life, and every call, written once over a leading stream axis --
    targets [streams, n], patterns [streams, T, n], outputs [streams, n, H, ...], state per stream.  SDRClassifierBank is this with
    its own axis; SDRClassifier is the one stream whose arguments and results come without the axis (_lift puts it on, _drop takes it
    off) and whose calls go through the one-stream C functions.  Neither is an instance of the other."""

    _create_name = None
    _prefix = None                              # of the C functions the calls go through: htm_classifier_ or htm_classifiers_
    _single = False                             # the public arrays come without the stream axis
    streams = 1
    source = None                               # SDRClassifierBank.shared(): the SDRClassifier whose weights the streams read

    def _create(self, engine, cfg, out):
        raise NotImplementedError

    def _pointers(self, a):
        """A call's device addresses -- one, or a sequence of `streams`; None: none -- as the update's C function takes them."""
        if self._single:
            return C.c_void_p(a) if a else None
        return (C.c_void_p * self.streams)(*[int(x) for x in a]) if a is not None else None

    def _no_shared_learning(self, learning):
        pass                                    # (SDRClassifierBank.shared() refuses here)

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

    def __init__(self, buckets=None, field=None, steps=(1,), alpha=0.001, shape=None):
        if (buckets is None) == (field is None):
            raise ValueError("SDRClassifier: give buckets= or field=, one of them")
        if field is not None and getattr(field, "kind_code", None) == FIELD_COORDINATE:
            raise ValueError("SDRClassifier: a coordinate field (or one of its axes) has no buckets to classify: give another field")
        self.field = field
        self.buckets, self.steps, self.alpha_q = check_params(field.buckets if buckets is None else buckets, steps, alpha)
        self.shape = None
        if shape is not None:
            self._set_shape(*shape)
        self.lib = None
        self.device = None
        self._clf = None
        self._last = None                       # weak reference to the engine of the last call
        self._home = None                       # a small model of the object's own, made when no other handle is there
        self._bufs = {}                         # the device buffers of a call's outputs and targets: name -> (address, words)
        self._pending = None                    # a state loaded before the object was bound

    def _set_shape(self, column_dim, cell_dim, max_pairs):
        column_dim, cell_dim, max_pairs = int(column_dim), int(cell_dim), int(max_pairs)
        if column_dim < 1 or not 1 <= cell_dim <= 64 or max_pairs < 1:
            raise ValueError(f"SDRClassifier: shape = (column_dim >= 1, cell_dim in [1, 64], max_pairs >= 1), got {(column_dim, cell_dim, max_pairs)}")
        shape = (column_dim, cell_dim, max_pairs)
        if self.shape is not None and self.shape != shape:
            raise ValueError(f"the classifier was made for patterns of shape {self.shape} (column_dim, cell_dim, pairs), this call has {shape}")
        self.shape = shape

    @property
    def units(self):
        return self.shape[0] * self.shape[1]

    @property
    def ring_len(self):
        return self.steps[-1] + 1

    # ---- binding
    def _bind(self, engine):
        if self.shape is None:
            raise RuntimeError("the classifier does not know the shape of its patterns yet: use it with a model, or give SDRClassifier(shape=)")
        if self._clf is None:
            self.lib = engine.lib
            cfg = L.HtmClassifierConfig(C.sizeof(L.HtmClassifierConfig), self.buckets, len(self.steps), self.alpha_q, self.units, self.shape[1],
                                        self.shape[2], (C.c_int32 * 8)(*self.steps))
            out = C.c_void_p()
            rc = self._create(engine, cfg, out)
            if rc != 0:
                raise HtmError(f"{self._create_name} failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")
            self._clf, self.device = out, engine.device
            self._last = weakref.ref(engine)
            if self._pending is not None:
                pending, self._pending = self._pending, None
                self._import(engine, pending)
        elif engine.device != self.device:
            raise ValueError(f"the classifier lives on device {self.device}, the model on device {engine.device}")
        # the library orders calls on one stream only: what the last engine enqueued is waited for before another engine touches the state
        last = self._last() if self._last is not None else None
        if last is not None and last is not engine and getattr(last, "h", None):
            last.sync()
        self._last = weakref.ref(engine)
        return engine

    def bind(self, model):
        """Bind the object to `model`'s device now -- and, unless it was given one, to the shape of the model's patterns -- and let
        the calls that need a handle of their own go through the model's.  Returns the object."""
        if self.shape is None:
            self._set_shape(*model_shape(model.engine))
        self._bind(model.engine)
        return self

    def _engine(self, device=None):
        engine = self._last() if self._last is not None else None
        if engine is not None and getattr(engine, "h", None) and device in (None, engine.device):
            return self._bind(engine)
        if self._clf is not None and device not in (None, self.device):
            raise ValueError(f"the classifier lives on device {self.device}, not {device}")
        if self._home is None:
            if device is None and self.device is None:
                raise RuntimeError("the classifier is not bound to a device yet: use it with a model, or give update_patterns(device=)")
            from .networks import HierarchicalTemporalMemory
            self._home = HierarchicalTemporalMemory(32, 64, 4, active_columns=4, device=self.device if device is None else int(device))
        return self._bind(self._home.engine)

    def __del__(self):
        clf, self._clf = getattr(self, "_clf", None), None
        if clf:
            self.lib.htm_classifier_destroy(clf)
        for ptr, _ in getattr(self, "_bufs", {}).values():
            self.lib.hipFree(ptr)

    def _check(self, engine, rc, what):
        if rc < 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")

    def _call(self, engine, name, *args):
        """The C function `name` of this object's set on (object, handle, *args)."""
        what = self._prefix + name
        self._check(engine, getattr(self.lib, what)(self._clf, engine.h, *args), what)

    def upload_targets(self, engine, targets):
        """int [n] -> the device address of the targets of a run's rows (kept until the next upload)."""
        self._bind(engine)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        ptr = engine.kept_buffer(self._bufs, "targets", max(targets.size, 1))
        engine._hip_check(self.lib.hipMemcpy(ptr, targets.ctypes.data_as(C.c_void_p), targets.nbytes, L.HIP_MEMCPY_HOST_TO_DEVICE), "hipMemcpy")
        return ptr

    def _weights(self, engine, name, i, h, rows):
        """read_weights or write_weights over the whole table of stream i's horizon h (the one-stream functions take no stream)."""
        self._call(engine, name, *(() if self._single else (i,)), h, 0, self.units, rows.ctypes.data_as(C.c_void_p))

    # ---- the update over device memory (what run() calls; nothing here waits)
    def pairs_buffer(self, engine, n):
        """The device address of a buffer for n steps' patterns of max_pairs pairs of every stream, [streams][n][max_pairs] (kept)."""
        self._bind(engine)
        return engine.kept_buffer(self._bufs, "pairs", 2 * self.streams * max(int(n), 1) * self.shape[2], spare=2)

    def enqueue(self, engine, device_pairs, pairs_per_step, n, device_targets, n_targets, first_step, device_resets, learning, distribution=False):
        """The update over n steps' patterns in device memory, enqueued on `engine`'s stream: device_pairs, device_targets and
        device_resets (or None) are device addresses, one each (SDRClassifier) or a sequence of `streams` each (a bank) -> nothing;
        read(engine, n, distribution) after the stream's wait gives the results."""
        self._no_shared_learning(learning)
        self._bind(engine)
        n, H, S = int(n), len(self.steps), self.streams
        best = engine.kept_buffer(self._bufs, "best", S * max(n, 1) * H * 2, spare=2)
        dist = engine.kept_buffer(self._bufs, "dist", S * max(n, 1) * H * self.buckets, spare=2) if distribution else None
        self._call(engine, "update", self._pointers(device_pairs), int(pairs_per_step), n, self._pointers(device_targets), int(n_targets), int(first_step),
                   self._pointers(device_resets), int(bool(learning)), C.c_void_p(best), C.c_void_p(dist) if dist else None)

    def read(self, engine, n, distribution=False):
        """(best int32 [streams, n, H, 2], dist int32 [streams, n, H, buckets] or None) of the last enqueue, after the engine's stream
        has been waited for (SDRClassifier: without the stream axis)."""
        n, H, S = int(n), len(self.steps), self.streams
        best = engine.read_words(self._bufs["best"][0], S * n * H * 2, np.int32).reshape(S, n, H, 2)
        dist = engine.read_words(self._bufs["dist"][0], S * n * H * self.buckets, np.int32).reshape(S, n, H, self.buckets) if distribution else None
        return self._drop(best), (self._drop(dist) if distribution else None)

    def check_targets(self, targets):
        """int [streams, n] (SDRClassifier: [n]) -> int32: -1 (any negative value) is missing; ValueError for a bucket at or above
        `buckets`."""
        t = np.asarray(targets)
        if t.ndim != (1 if self._single else 2) or self._lift(t).shape[0] != self.streams or t.dtype.kind not in "iu":
            raise ValueError(f"targets: int {self._dims('n')}, got {t.dtype} {list(t.shape)}")
        if t.size and int(t.max()) >= self.buckets:
            raise ValueError(f"targets: bucket {int(t.max())} is at or above buckets = {self.buckets}")
        return np.ascontiguousarray(np.where(t < 0, -1, t).astype(np.int32))

    # ---- the stand-alone door
    def update_patterns(self, index, words, targets, learning=True, resets=None, device=None, distribution=True):
        """T further steps of every stream from their patterns: index int [streams, T, n], words uint32 [streams, T, n] (pair j of step
        t is (index[.., t, j], words[.., t, j]); a negative index or a zero word contributes nothing), targets int [streams, T] (-1:
        missing), resets bool [streams, T] or None; SDRClassifier: all without the stream axis.  Checked here: the indices of a step
        are distinct and inside the table, no word has a bit at or above cell_dim, n <= max_pairs.  -> (best int32 [streams, T, H, 2]
        as (bucket, p in units of 2^-16), dist int32 [streams, T, H, buckets] or None)."""
        self._no_shared_learning(learning)
        if self.shape is None:
            raise RuntimeError(f"the classifier does not know the shape of its patterns yet: use it with a model, or give {type(self).__name__}(shape=)")
        index, words = np.asarray(index), np.asarray(words)
        S = self.streams
        if not self._single and (index.ndim != 3 or index.shape[0] != S or words.shape != index.shape):
            raise ValueError(f"patterns: index int [{S}, T, n] and words uint32 [{S}, T, n], got {list(index.shape)} and {list(words.shape)}")
        checked = [check_patterns(i, w, self.units, self.shape[1]) for i, w in zip(self._lift(index), self._lift(words))]
        index, words = np.stack([c[0] for c in checked]), np.stack([c[1] for c in checked])
        _, T, n = index.shape
        if not 1 <= n <= self.shape[2]:
            raise ValueError(f"patterns: 1 to max_pairs = {self.shape[2]} pairs per step, got {n}")
        targets = self._lift(self.check_targets(targets))
        if targets.shape != (S, T):
            raise ValueError(f"targets: int {self._dims(T)}, got {list(self._drop(targets).shape)}")
        if resets is not None:
            resets = np.asarray(resets, dtype=np.bool_)
            resets = self._lift(resets.ravel() if self._single else resets)
            if resets.shape != (S, T):
                raise ValueError(f"resets: bool {self._dims(T)}, got {list(self._drop(resets).shape)}")
        H = len(self.steps)
        if T == 0:
            return self._drop(np.zeros((S, 0, H, 2), np.int32)), (self._drop(np.zeros((S, 0, H, self.buckets), np.int32)) if distribution else None)
        engine = self._engine(device)
        pairs = np.empty((S, T, n, 2), dtype=np.int32)
        pairs[..., 0], pairs[..., 1] = index, words.view(np.int32)
        buf = engine.device_buffer(pairs.nbytes, pairs)
        tbuf = engine.device_buffer(targets.nbytes, targets)
        rbuf, rtab = None, None
        try:
            if resets is not None:
                row = (T + 31) // 32 * 4
                bits = np.zeros((S, row), dtype=np.uint8)
                pb = np.packbits(resets, axis=1, bitorder="little")
                bits[:, :pb.shape[1]] = pb
                rbuf = engine.device_buffer(bits.nbytes, bits)
                rtab = self._drop([rbuf + i * row for i in range(S)])
            self.enqueue(engine, self._drop([buf + i * T * n * 8 for i in range(S)]), n, T, self._drop([tbuf + i * T * 4 for i in range(S)]), T, 0, rtab, learning,
                         distribution)
            engine.sync()
            best, dist = self.read(engine, T, distribution)
            return best.copy(), (dist.copy() if dist is not None else None)
        finally:
            engine.sync()
            for p in (buf, tbuf, rbuf):
                if p:
                    self.lib.hipFree(p)

    # ---- reset, state: kept with the stream axis (count [streams], ring [streams, ...], weights [tables, ...]), also while pending
    def _reset(self, flags, *args):
        """Empty the history of every stream, or of those `flags` (bool [streams]) names; args: what the C call takes for them."""
        if self._clf is None:
            if self._pending is not None:
                self._pending["count"] = np.where(flags, 0, self._pending["count"]) if flags is not None else np.zeros(self.streams, np.int64)
            return
        self._call(self._engine(), "reset", *args)

    @property
    def _tables(self):
        """Weight tables a state holds: one per stream, or the owner's one."""
        return 1 if self.source is not None else self.streams

    def _empty_state(self):
        ring = np.zeros((self.streams, self.ring_len, self.shape[2], 2), dtype=np.int32)
        ring[..., 0] = -1
        return dict(total=np.int64(0), count=np.zeros(self.streams, np.int64), ring=ring,
                    weights=np.zeros((self._tables, len(self.steps), self.units, self.buckets), np.int32))

    def _params(self):
        return self._axis + (self.buckets, self.alpha_q) + (self.shape or ()) + self.steps

    def state_dict(self):
        """{"params": int64 [streams, buckets, alpha_q, column_dim, cell_dim, max_pairs, steps...], "total": int64, "count": int64
        [streams], "ring": int32 [streams, ring_len, max_pairs, 2], "weights": int32 [streams, H, units, buckets]} -- the whole state,
        read from the device (shared(): "weights" is the owner's table, once: [1, H, units, buckets]; SDRClassifier: no streams in
        "params" and no stream axis, "count" one int64).  Dense: H x units x buckets x 4 bytes of host memory per table (16 MiB per
        horizon at 2 048 x 32 units and 64 buckets): meant for small models."""
        if self.shape is None:
            raise RuntimeError("the classifier does not know the shape of its patterns yet")
        if self._clf is None and self.source is not None:          # (the weights are the owner's, on its device: bound through its engine)
            self._engine()
        if self._clf is None:
            state = self._pending if self._pending is not None else self._empty_state()
        else:
            engine = self._engine()
            S, H = self.streams, len(self.steps)
            size = 8 + S * 8 + S * self.ring_len * self.shape[2] * 8
            assert size == getattr(self.lib, self._prefix + "state_bytes")(self._clf)
            blob = np.zeros(size, dtype=np.uint8)
            self._call(engine, "export", blob.ctypes.data_as(C.c_void_p), size)
            head = blob[:8 + S * 8].view(np.int64)
            weights = np.zeros((self._tables, H, self.units, self.buckets), dtype=np.int32)
            for i in range(self._tables):
                for h in range(H):
                    self._weights(engine, "read_weights", i, h, weights[i, h])
            state = dict(total=np.int64(head[0]), count=head[1:], ring=blob[8 + S * 8:].view(np.int32).reshape(S, self.ring_len, self.shape[2], 2), weights=weights)
        out = {k: np.array(v if k == "total" else self._drop(v))[()] for k, v in state.items()}       # (copies; [()]: a scalar of a 0-d array)
        return dict(out, params=np.asarray(self._params(), dtype=np.int64))

    def load_state_dict(self, state):
        """The state of a state_dict() of an object with the same parameters and shape (shared(): the weights are the owner's and are
        not written)."""
        params = tuple(int(x) for x in state["params"])
        at = 2 if self._single else 3
        if self.shape is None and len(params) == at + 3 + len(self.steps):
            self._set_shape(*params[at:at + 3])
        if params != self._params():
            raise ValueError(f"the state was saved with parameters {params} ({'' if self._single else 'streams, '}buckets, alpha_q, column_dim, cell_dim, max_pairs, "
                             f"steps...), this object has {self._params()}")
        S, tables = self.streams, self._tables
        total = int(state["total"])
        count = self._lift(np.asarray(state["count"], dtype=np.int64))
        if count.shape != (S,) or (count < 0).any() or (count > total).any():
            raise ValueError(f"state: count int64 {self._dims()} with 0 <= count <= total, got {count.tolist()}, total {total}")
        ring = self._lift(np.ascontiguousarray(state["ring"], dtype=np.int32))
        weights = self._lift(np.ascontiguousarray(state["weights"], dtype=np.int32))
        for name, a, want in (("ring", ring, (S, self.ring_len, self.shape[2], 2)), ("weights", weights, (tables, len(self.steps), self.units, self.buckets))):
            if a.shape != want:
                raise ValueError(f"state['{name}']: int32 {list(want[self._single:])}, got {list(self._drop(a).shape)}")
        if weights.size and (weights.max() > W_LIMIT or weights.min() < -W_LIMIT):
            raise ValueError("state['weights']: a weight is outside [-2^30, 2^30]")
        clean = dict(total=np.int64(total), count=count.copy(), ring=ring.copy(), weights=weights.copy())
        if self._clf is None:
            self._pending = clean
        else:
            self._import(self._engine(), clean)

    def _import(self, engine, state):
        S = self.streams
        blob = np.zeros(8 + S * 8 + state["ring"].nbytes, dtype=np.uint8)
        head = blob[:8 + S * 8].view(np.int64)
        head[0], head[1:] = state["total"], state["count"]
        blob[8 + S * 8:] = state["ring"].view(np.uint8).ravel()
        self._call(engine, "import", blob.ctypes.data_as(C.c_void_p), blob.size)
        if self.source is not None:
            return
        for i in range(S):
            for h in range(len(self.steps)):
                self._weights(engine, "write_weights", i, h, np.ascontiguousarray(state["weights"][i, h]))


class SDRClassifier(_DeviceClassifier):
    """The classifier of `buckets` buckets (or of an encoder field's: `field`, whose value_of also names the values) for the
    horizons `steps` with learning rate `alpha`.  The shape of the patterns -- units = column_dim * cell_dim, cell_dim, and the pairs
    a pattern has at most -- comes from the model of the first run(classifier=), or from `shape=(column_dim, cell_dim, max_pairs)`
    for stand-alone use.  The object binds to a device lazily, as AnomalyLikelihood does; every update continues where the last one
    ended, whichever door it came through.  The calls are _DeviceClassifier's for one stream, without the stream axis: targets int
    [n], patterns [T, n], best [n, H, 2], a state of "count": int64 and "ring": int32 [ring_len, max_pairs, 2]."""

    _create_name = "htm_classifier_create"
    _prefix = "htm_classifier_"
    _single = True

    def _create(self, engine, cfg, out):
        return self.lib.htm_classifier_create(engine.h, C.byref(cfg), EXP_TABLE.ctypes.data_as(C.c_void_p), C.byref(out))

    def reset(self):
        """Empty the history: the next steps learn nothing from the patterns before them (the weights stay)."""
        self._reset(None)


class SDRClassifierBank(_DeviceClassifier):
    """`streams` independent SDRClassifier streams of one config in one device object (htm_classifiers_*): stream
    i fed (patterns_i, targets_i, resets_i) equals an SDRClassifier fed the same, bit for bit, and every call steps all streams in
    the launches of one -- two per step when learning, one per chunk of steps otherwise, whatever `streams` is.

        bank = SDRClassifierBank(64, buckets=50, steps=(1, 5), shape=(2048, 32, 40))
        best, dist = bank.update_patterns(index, words, targets)        # index, words [64, T, P], targets [64, T]
        views = SDRClassifierBank.shared(clf, 4)                        # four frozen streams over clf's weights, read where they lie

    Memory: streams x the one-stream object's, except shared(), which adds only rings, counts and accumulators."""

    _create_name = "htm_classifiers_create"
    _prefix = "htm_classifiers_"

    def __init__(self, streams, buckets=None, field=None, steps=(1,), alpha=0.001, shape=None):
        super().__init__(buckets=buckets, field=field, steps=steps, alpha=alpha, shape=shape)
        self._set_streams(streams)

    def _set_streams(self, streams):
        self.streams = int(streams)
        if not 1 <= self.streams <= 65535 // len(self.steps):
            raise ValueError(f"SDRClassifierBank: streams must be in [1, 65535 // len(steps) = {65535 // len(self.steps)}], got {streams}")

    @classmethod
    def shared(cls, clf, streams):
        """A bank of `streams` frozen streams that read the weights of `clf`, a bound SDRClassifier: no copy -- what clf learns later
        (through htm.run(classifier=clf), say) the next call here sees.  The bank keeps a reference to clf; its own state is the
        streams' histories.  Learning through the bank is refused."""
        if not isinstance(clf, SDRClassifier):
            raise ValueError("SDRClassifierBank.shared(): clf is a one-stream SDRClassifier")
        if clf._clf is None:
            raise ValueError("SDRClassifierBank.shared(): clf is not bound to a device yet (use it with a model, or clf.bind(model))")
        bank = cls.__new__(cls)
        _DeviceClassifier.__init__(bank, buckets=clf.buckets, steps=clf.steps, shape=clf.shape)
        bank.field, bank.alpha_q = clf.field, clf.alpha_q
        bank._set_streams(streams)
        bank.source = clf
        bank._last = clf._last                  # (its calls go through the engine clf's last call came through, until a model brings its own)
        return bank

    def _create(self, engine, cfg, out):
        share = None
        if self.source is not None:
            if self.source._clf is None or self.source.device != engine.device:
                raise ValueError(f"the shared classifier lives on device {self.source.device}, the model on device {engine.device}")
            share = self.source._clf
        return self.lib.htm_classifiers_create(engine.h, C.byref(cfg), EXP_TABLE.ctypes.data_as(C.c_void_p), self.streams, share, C.byref(out))

    def _bind(self, engine):
        if self.source is not None:             # (what the owner's last engine enqueued on the weights is waited for first)
            owner = self.source._last() if self.source._last is not None else None
            if owner is not None and owner is not engine and getattr(owner, "h", None):
                owner.sync()
        return super()._bind(engine)

    def _no_shared_learning(self, learning):
        if learning and self.source is not None:
            raise ValueError("SDRClassifierBank.shared(): the streams read one weight table -- learning is refused (the owner learns through its own calls)")

    def reset(self, streams=None):
        """Empty the history of every stream, or of those `streams` (bool [streams]) names (the weights stay)."""
        flags = None
        if streams is not None:
            flags = np.ascontiguousarray(np.asarray(streams, dtype=np.bool_).ravel()).astype(np.uint8)
            if flags.shape != (self.streams,):
                raise ValueError(f"streams: bool [{self.streams}], got {list(flags.shape)}")
        self._reset(flags, flags.ctypes.data_as(C.c_void_p) if flags is not None else None)


def model_shape(engine):
    """(column_dim, cell_dim, pairs per captured step) of an engine's patterns."""
    return engine.column_dim, engine.cell_dim, engine.active_columns * ((engine.cell_dim + 31) // 32)
