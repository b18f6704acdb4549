"""AnomalyLikelihood: the anomaly likelihood of many streams kept on the device (htm_likelihood_*, include/bithtm_hip.h;
DESIGN.md section 22).  The definition is likelihood.py; the device equals it bit for bit.

    lk = AnomalyLikelihood(streams=64)                      # NuPIC's defaults; bound to a device at first use
    recs = group.run(inputs, steps, likelihood=lk)          # recs[i].anomaly_likelihood float64[steps], .log_likelihood
    tick = group.tick(values, encoder=enc, likelihood=lk)   # tick.anomaly_likelihood float64[64]: one launch more per tick
    rec = model.run(inputs, steps, likelihood=AnomalyLikelihood())          # one stream

Sequence resets of a model do not touch the likelihood's state; lk.reset() does."""

import ctypes as C
import weakref

import numpy as np

from . import _lib as L
from .engine import RECORD_COUNTERS, HtmError
from .likelihood import PARAMETERS, TAIL, check_counts, check_params

_ACTIVE, _BURSTING = RECORD_COUNTERS.index("active_columns"), RECORD_COUNTERS.index("bursting_columns")


class AnomalyLikelihood:
    """The likelihood state of `streams` streams with the parameters of likelihood.check_params (NuPIC's names and defaults:
    learning_period=288, estimation_samples=100, history=8640, averaging_window=10, reestimation_period=100).  The object binds
    to a device lazily: at its first use with a model (run / group.run / group.tick with likelihood=) or on
    update_counts(device=).  Every update continues where the last one ended, whichever door it came through."""

    def __init__(self, streams=1, **params):
        self.streams = int(streams)
        if self.streams < 1:
            raise ValueError(f"streams must be at least 1, got {streams}")
        self.params = check_params(**params)
        self.lib = None
        self.device = None
        self._lk = None
        self._last = None                       # weak reference to the engine of the last call (its handle serves reset / state_dict)
        self._home = None                       # a small model of the object's own, made when no other handle is there
        self._out = (None, 0)                   # the device buffer of a call's likelihoods (address, doubles)
        self._pending = None                    # a state loaded before the object was bound

    # ---- binding
    def _bind(self, engine):
        if self._lk is None:
            self.lib = engine.lib
            cfg = L.HtmLikelihoodConfig(C.sizeof(L.HtmLikelihoodConfig), *self.params)
            out = C.c_void_p()
            rc = self.lib.htm_likelihood_create(engine.h, C.byref(cfg), TAIL.ctypes.data_as(C.c_void_p), self.streams, C.byref(out))
            if rc != 0:
                raise HtmError(f"htm_likelihood_create failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")
            self._lk, self.device = out, engine.device
            if self._pending is not None:
                pending, self._pending = self._pending, None
                self._import(engine, pending)
        elif engine.device != self.device:
            raise ValueError(f"the likelihood object lives on device {self.device}, the model on device {engine.device}")
        # the library orders calls on one stream only: what the last engine enqueued is waited for before another engine -- which
        # may enqueue on another stream -- touches the state (an engine that is gone has waited for its stream in htm_destroy)
        last = self._last() if self._last is not None else None
        if last is not None and last is not engine and getattr(last, "h", None):
            last.sync()
        self._last = weakref.ref(engine)
        return engine

    def bind(self, model):
        """Bind the object to `model`'s device now, and let the calls that need a handle of their own (update_counts, reset,
        state_dict) go through the model's instead of a small model of the object's own.  Returns the object."""
        self._bind(model.engine)
        return self

    def _engine(self, device=None):
        """An engine whose handle the next call goes through: the last one used if it is still there, else a small model of the
        object's own on `device` (or on the object's device)."""
        engine = self._last() if self._last is not None else None
        if engine is not None and getattr(engine, "h", None) and device in (None, engine.device):
            return self._bind(engine)
        if self._lk is not None and device not in (None, self.device):
            raise ValueError(f"the likelihood object lives on device {self.device}, not {device}")
        if self._home is None:
            if device is None and self.device is None:
                raise RuntimeError("the likelihood object is not bound to a device yet: use it with a model, or give update_counts(device=)")
            from .networks import HierarchicalTemporalMemory
            self._home = HierarchicalTemporalMemory(32, 64, 4, active_columns=4, device=self.device if device is None else int(device))
        return self._bind(self._home.engine)

    def __del__(self):
        lk, self._lk = getattr(self, "_lk", None), None
        if lk:
            self.lib.htm_likelihood_destroy(lk)
        ptr = getattr(self, "_out", (None, 0))[0]
        if ptr:
            self.lib.hipFree(ptr)

    def _check(self, engine, rc, what):
        if rc < 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.htm_last_error(engine.h).decode()}")

    # ---- the update behind recorded steps (what run(), group.run() call; nothing here waits)
    def enqueue(self, engine, record_ptrs, n):
        """htm_likelihood_update over the device record buffers `record_ptrs` (one per stream, n htm_step_record each), enqueued on
        `engine`'s stream -> nothing; read(engine, n) after the stream's wait gives float64 [streams, n]."""
        if len(record_ptrs) != self.streams:
            raise ValueError(f"the likelihood object has {self.streams} streams, the call {len(record_ptrs)}")
        self._bind(engine)
        n = int(n)
        ptr, size = self._out
        if size < self.streams * max(n, 1):
            if ptr:
                engine.sync()
                self.lib.hipFree(ptr)
            size = max(self.streams * max(n, 1), 2 * size)
            ptr = engine.device_buffer(8 * size)
            self._out = (ptr, size)
        table = (C.c_void_p * self.streams)(*record_ptrs)
        self._check(engine, self.lib.htm_likelihood_update(self._lk, engine.h, table, n, C.c_void_p(ptr)), "htm_likelihood_update")

    def read(self, engine, n):
        """The likelihoods of the last enqueue(engine, ..., n), float64 [streams, n], after the engine's stream has been waited for."""
        words = engine.read_words(self._out[0], 2 * self.streams * int(n), np.uint32)
        return words.view(np.float64).reshape(self.streams, int(n))

    # ---- the stand-alone door
    def update_counts(self, active, bursting, device=None):
        """The likelihoods of T further steps of every stream from their counts: int arrays [streams, T] (or [T] for one stream),
        0 <= bursting <= active < 2^24, checked here.  They are uploaded as records, htm_likelihood_update runs over them and
        the result comes back: float64 of the counts' shape."""
        active, bursting = check_counts(active, bursting)
        shape = active.shape
        if active.ndim == 1 and self.streams == 1:
            active, bursting = active[None], bursting[None]
        if active.ndim != 2 or active.shape[0] != self.streams:
            raise ValueError(f"counts: int [{self.streams}, T], got {shape}")
        engine = self._engine(device)
        T = active.shape[1]
        if T == 0:
            return np.zeros(shape, dtype=np.float64)
        records = np.zeros((self.streams, T, len(RECORD_COUNTERS)), dtype=np.int32)
        records[:, :, _ACTIVE], records[:, :, _BURSTING] = active, bursting
        buf = engine.device_buffer(records.nbytes, records)
        try:
            stride = T * len(RECORD_COUNTERS) * 4
            self.enqueue(engine, [buf + i * stride for i in range(self.streams)], T)
            engine.sync()
            return self.read(engine, T).reshape(shape).copy()
        finally:
            self.lib.hipFree(buf)

    # ---- reset, state
    def reset(self, streams=None):
        """The flagged streams (bool [streams]; None: all) start again at t = 0: no history, no estimate."""
        if streams is not None:
            streams = np.asarray(streams)
            if streams.shape != (self.streams,):
                raise ValueError(f"streams: bool [{self.streams}], got shape {streams.shape}")
            streams = np.ascontiguousarray(streams.astype(np.bool_), dtype=np.uint8)
        if self._lk is None:
            if self._pending is not None:
                fresh = _empty_state(self.streams, self.params)
                for i in range(self.streams):
                    if streams is None or streams[i]:
                        for key in fresh:
                            self._pending[key][i] = fresh[key][i]
            return
        engine = self._engine()
        self._check(engine, self.lib.htm_likelihood_reset(self._lk, engine.h, None if streams is None else streams.ctypes.data_as(C.c_void_p)),
                    "htm_likelihood_reset")

    def _layout(self):
        """(name, dtype, shape, byte offset) of the parts of the exported state (include/bithtm_hip.h), and its size."""
        n, (_, _, hist, w, _) = self.streams, self.params
        parts, at = [], 0
        for name, dtype, shape in (("t", np.int64, (n,)), ("mean", np.float64, (n,)), ("std", np.float64, (n,)), ("has_estimate", np.int32, (n,)),
                                   ("q_ring", np.int32, (n, w)), ("a_ring", np.int32, (n, hist))):
            parts.append((name, dtype, shape, at))
            at += int(np.prod(shape)) * np.dtype(dtype).itemsize
            if name in ("has_estimate", "a_ring"):      # (the flags and the whole state are padded to a multiple of 8 bytes)
                at = (at + 7) & ~7
        return parts, at

    def state_dict(self):
        """{"params": int64[5], "t": int64[streams], "mean", "std": float64[streams], "has_estimate": int32[streams], "q_ring":
        int32[streams, averaging_window], "a_ring": int32[streams, history]} -- the whole state, read from the device."""
        if self._lk is None:
            state = self._pending if self._pending is not None else _empty_state(self.streams, self.params)
            return dict({k: v.copy() for k, v in state.items()}, params=np.asarray(self.params, dtype=np.int64))
        engine = self._engine()
        parts, size = self._layout()
        assert size == self.lib.htm_likelihood_state_bytes(self._lk), (size, self.lib.htm_likelihood_state_bytes(self._lk))
        blob = np.zeros(size, dtype=np.uint8)
        self._check(engine, self.lib.htm_likelihood_export(self._lk, engine.h, blob.ctypes.data_as(C.c_void_p), size), "htm_likelihood_export")
        state = {name: blob[at:at + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape).copy() for name, dtype, shape, at in parts}
        state["params"] = np.asarray(self.params, dtype=np.int64)
        return state

    def load_state_dict(self, state):
        """The state of a state_dict() of an object with the same streams and parameters."""
        if tuple(int(x) for x in state["params"]) != self.params:
            raise ValueError(f"the state was saved with parameters {dict(zip(PARAMETERS, state['params']))}, this object has {dict(zip(PARAMETERS, self.params))}")
        parts, _ = self._layout()
        clean = {}
        for name, dtype, shape, _ in parts:
            value = np.ascontiguousarray(state[name], dtype=dtype)
            if value.shape != shape:
                raise ValueError(f"state[{name!r}]: {dtype.__name__} {list(shape)}, got {list(value.shape)}")
            clean[name] = value.copy()
        if (clean["t"] < 0).any():
            raise ValueError("state['t'] must not be negative")
        if self._lk is None:
            self._pending = clean
        else:
            self._import(self._engine(), clean)

    def _import(self, engine, state):
        parts, size = self._layout()
        blob = np.zeros(size, dtype=np.uint8)
        for name, dtype, shape, at in parts:
            raw = state[name].view(np.uint8).ravel()
            blob[at:at + raw.size] = raw
        self._check(engine, self.lib.htm_likelihood_import(self._lk, engine.h, blob.ctypes.data_as(C.c_void_p), size), "htm_likelihood_import")


def _empty_state(streams, params):
    _, _, hist, w, _ = params
    return dict(t=np.zeros(streams, np.int64), mean=np.zeros(streams, np.float64), std=np.zeros(streams, np.float64),
                has_estimate=np.zeros(streams, np.int32), q_ring=np.zeros((streams, w), np.int32), a_ring=np.zeros((streams, hist), np.int32))
