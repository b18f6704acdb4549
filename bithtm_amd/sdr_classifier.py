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
from .engine import HtmError


class SDRClassifier:
    """The classifier of `buckets` buckets (or of an encoder field's: `field`, whose value_of also names the values) for the
    horizons `steps` with learning rate `alpha`.  The shape of the patterns -- units = column_dim * cell_dim, cell_dim, and the pairs
    a pattern has at most -- comes from the model of the first run(classifier=), or from `shape=(column_dim, cell_dim, max_pairs)`
    for stand-alone use.  The object binds to a device lazily, as AnomalyLikelihood does; every update continues where the last one
    ended, whichever door it came through."""

    def __init__(self, buckets=None, field=None, steps=(1,), alpha=0.001, shape=None):
        if (buckets is None) == (field is None):
            raise ValueError("SDRClassifier: give buckets= or field=, one of them")
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
            rc = self.lib.htm_classifier_create(engine.h, C.byref(cfg), EXP_TABLE.ctypes.data_as(C.c_void_p), C.byref(out))
            if rc != 0:
                raise HtmError(f"htm_classifier_create failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")
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

    # ---- the update behind captured steps (what run() calls; nothing here waits)
    def upload_targets(self, engine, targets):
        """int [n] -> the device address of the targets of a run's rows (kept until the next upload)."""
        self._bind(engine)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        ptr = engine.kept_buffer(self._bufs, "targets", max(targets.size, 1))
        engine._hip_check(self.lib.hipMemcpy(ptr, targets.ctypes.data_as(C.c_void_p), targets.nbytes, L.HIP_MEMCPY_HOST_TO_DEVICE), "hipMemcpy")
        return ptr

    def pairs_buffer(self, engine, n):
        """The device address of a buffer for n steps' patterns of max_pairs pairs (kept)."""
        self._bind(engine)
        return engine.kept_buffer(self._bufs, "pairs", 2 * max(int(n), 1) * self.shape[2], spare=2)

    def enqueue(self, engine, device_pairs, pairs_per_step, n, device_targets, n_targets, first_step, device_resets, learning, distribution=False):
        """htm_classifier_update over n steps' patterns in device memory, enqueued on `engine`'s stream -> nothing; read(engine, n,
        distribution) after the stream's wait gives the results."""
        self._bind(engine)
        n, H = int(n), len(self.steps)
        best = engine.kept_buffer(self._bufs, "best", max(n, 1) * H * 2, spare=2)
        dist = engine.kept_buffer(self._bufs, "dist", max(n, 1) * H * self.buckets, spare=2) if distribution else None
        self._check(engine, self.lib.htm_classifier_update(self._clf, engine.h, C.c_void_p(device_pairs), int(pairs_per_step), n, C.c_void_p(device_targets),
                                                           int(n_targets), int(first_step), C.c_void_p(device_resets) if device_resets else None,
                                                           int(bool(learning)), C.c_void_p(best), C.c_void_p(dist) if dist else None),
                    "htm_classifier_update")

    def read(self, engine, n, distribution=False):
        """(best int32 [n, H, 2], dist int32 [n, H, buckets] or None) of the last enqueue, after the engine's stream has been waited for."""
        n, H = int(n), len(self.steps)
        best = engine.read_words(self._bufs["best"][0], n * H * 2, np.int32).reshape(n, H, 2)
        dist = engine.read_words(self._bufs["dist"][0], n * H * self.buckets, np.int32).reshape(n, H, self.buckets) if distribution else None
        return best, dist

    def check_targets(self, targets):
        """int [n] -> int32 [n]: -1 (any negative value) is missing; ValueError for a bucket at or above `buckets`."""
        t = np.asarray(targets)
        if t.ndim != 1 or t.dtype.kind not in "iu":
            raise ValueError(f"targets: int [n], got {t.dtype} {list(t.shape)}")
        if t.size and int(t.max()) >= self.buckets:
            raise ValueError(f"targets: bucket {int(t.max())} is at or above buckets = {self.buckets}")
        return np.where(t < 0, -1, t).astype(np.int32)

    # ---- the stand-alone door
    def update_patterns(self, index, words, targets, learning=True, resets=None, device=None, distribution=True):
        """T further steps from their patterns: index int [T, n], words uint32 [T, n] (pair j of step t is (index[t, j], words[t, j]);
        a negative index or a zero word contributes nothing), targets int [T] (-1: missing), resets bool [T] or None.  Checked here:
        the indices of a step are distinct and inside the table, no word has a bit at or above cell_dim, n <= max_pairs.  ->
        (best int32 [T, H, 2] as (bucket, p in units of 2^-16), dist int32 [T, H, buckets] or None)."""
        if self.shape is None:
            raise RuntimeError("the classifier does not know the shape of its patterns yet: use it with a model, or give SDRClassifier(shape=)")
        index, words = check_patterns(index, words, self.units, self.shape[1])
        T, n = index.shape
        if not 1 <= n <= self.shape[2]:
            raise ValueError(f"patterns: 1 to max_pairs = {self.shape[2]} pairs per step, got {n}")
        targets = self.check_targets(targets)
        if targets.shape != (T,):
            raise ValueError(f"targets: int [{T}], got {list(targets.shape)}")
        if resets is not None:
            resets = np.asarray(resets, dtype=np.bool_).ravel()
            if resets.shape != (T,):
                raise ValueError(f"resets: bool [{T}], got {list(resets.shape)}")
        H = len(self.steps)
        if T == 0:
            return np.zeros((0, H, 2), np.int32), (np.zeros((0, H, self.buckets), np.int32) if distribution else None)
        engine = self._engine(device)
        pairs = np.empty((T, n, 2), dtype=np.int32)
        pairs[:, :, 0], pairs[:, :, 1] = index, words.view(np.int32)
        buf = engine.device_buffer(pairs.nbytes, pairs)
        tbuf = engine.device_buffer(targets.nbytes, targets)
        rbuf = None
        try:
            if resets is not None:
                bits = np.zeros((T + 31) // 32 * 4, dtype=np.uint8)
                pb = np.packbits(resets, bitorder="little")
                bits[:pb.size] = pb
                rbuf = engine.device_buffer(bits.nbytes, bits)
            self.enqueue(engine, buf, n, T, tbuf, T, 0, rbuf, learning, distribution)
            engine.sync()
            best, dist = self.read(engine, T, distribution)
            return best.copy(), (dist.copy() if dist is not None else None)
        finally:
            engine.sync()
            for p in (buf, tbuf, rbuf):
                if p:
                    self.lib.hipFree(p)

    # ---- reset, state
    def reset(self):
        """Empty the history: the next steps learn nothing from the patterns before them (the weights stay)."""
        if self._clf is None:
            if self._pending is not None:
                self._pending["count"] = np.int64(0)
            return
        engine = self._engine()
        self._check(engine, self.lib.htm_classifier_reset(self._clf, engine.h), "htm_classifier_reset")

    def _empty_state(self):
        ring = np.zeros((self.ring_len, self.shape[2], 2), dtype=np.int32)
        ring[:, :, 0] = -1
        return dict(total=np.int64(0), count=np.int64(0), ring=ring, weights=np.zeros((len(self.steps), self.units, self.buckets), np.int32))

    def state_dict(self):
        """{"params": int64 [buckets, alpha_q, column_dim, cell_dim, max_pairs, steps...], "total", "count": int64, "ring": int32
        [ring_len, max_pairs, 2], "weights": int32 [H, units, buckets]} -- the whole state, read from the device.  Dense: H x units x
        buckets x 4 bytes of host memory (16 MiB per horizon at 2 048 x 32 units and 64 buckets): meant for small models."""
        if self.shape is None:
            raise RuntimeError("the classifier does not know the shape of its patterns yet")
        params = np.asarray((self.buckets, self.alpha_q) + self.shape + self.steps, dtype=np.int64)
        if self._clf is None:
            state = self._pending if self._pending is not None else self._empty_state()
            return dict({k: np.array(v) for k, v in state.items()}, params=params)
        engine = self._engine()
        size = 16 + self.ring_len * self.shape[2] * 8
        assert size == self.lib.htm_classifier_state_bytes(self._clf)
        blob = np.zeros(size, dtype=np.uint8)
        self._check(engine, self.lib.htm_classifier_export(self._clf, engine.h, blob.ctypes.data_as(C.c_void_p), size), "htm_classifier_export")
        head = blob[:16].view(np.int64)
        weights = np.zeros((len(self.steps), self.units, self.buckets), dtype=np.int32)
        for h in range(len(self.steps)):
            self._check(engine, self.lib.htm_classifier_read_weights(self._clf, engine.h, h, 0, self.units, weights[h].ctypes.data_as(C.c_void_p)),
                        "htm_classifier_read_weights")
        return dict(params=params, total=np.int64(head[0]), count=np.int64(head[1]),
                    ring=blob[16:].view(np.int32).reshape(self.ring_len, self.shape[2], 2).copy(), weights=weights)

    def load_state_dict(self, state):
        """The state of a state_dict() of an object with the same parameters and shape."""
        params = tuple(int(x) for x in state["params"])
        if self.shape is None and len(params) == 5 + len(self.steps):
            self._set_shape(*params[2:5])
        mine = (self.buckets, self.alpha_q) + (self.shape or ()) + self.steps
        if params != mine:
            raise ValueError(f"the state was saved with parameters {params} (buckets, alpha_q, column_dim, cell_dim, max_pairs, steps...), this object has {mine}")
        total, count = int(state["total"]), int(state["count"])
        if not 0 <= count <= total:
            raise ValueError(f"state: 0 <= count <= total, got count {count}, total {total}")
        ring = np.ascontiguousarray(state["ring"], dtype=np.int32)
        weights = np.ascontiguousarray(state["weights"], dtype=np.int32)
        if ring.shape != (self.ring_len, self.shape[2], 2):
            raise ValueError(f"state['ring']: int32 {[self.ring_len, self.shape[2], 2]}, got {list(ring.shape)}")
        if weights.shape != (len(self.steps), self.units, self.buckets):
            raise ValueError(f"state['weights']: int32 {[len(self.steps), self.units, self.buckets]}, got {list(weights.shape)}")
        if weights.size and (weights.max() > W_LIMIT or weights.min() < -W_LIMIT):
            raise ValueError("state['weights']: a weight is outside [-2^30, 2^30]")
        clean = dict(total=np.int64(total), count=np.int64(count), ring=ring.copy(), weights=weights.copy())
        if self._clf is None:
            self._pending = clean
        else:
            self._import(self._engine(), clean)

    def _import(self, engine, state):
        blob = np.zeros(16 + state["ring"].nbytes, dtype=np.uint8)
        blob[:16].view(np.int64)[:] = (state["total"], state["count"])
        blob[16:] = state["ring"].view(np.uint8).ravel()
        self._check(engine, self.lib.htm_classifier_import(self._clf, engine.h, blob.ctypes.data_as(C.c_void_p), blob.size), "htm_classifier_import")
        for h in range(len(self.steps)):
            w = np.ascontiguousarray(state["weights"][h])
            self._check(engine, self.lib.htm_classifier_write_weights(self._clf, engine.h, h, 0, self.units, w.ctypes.data_as(C.c_void_p)),
                        "htm_classifier_write_weights")


def model_shape(engine):
    """(column_dim, cell_dim, pairs per captured step) of an engine's patterns."""
    return engine.column_dim, engine.cell_dim, engine.active_columns * ((engine.cell_dim + 31) // 32)
