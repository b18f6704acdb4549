"""Counterparts of bithtm/regularizations.py with the same constructor signatures.

Inside a SpatialPooler the computation they describe runs in the HIP engine's fused timestep (kernels
`k_sp_overlap`, `k_sel_pass`, `k_sp_emit`) and these objects carry the parameters and expose the state.  Called on
their own -- `process(...)` / `update(...)` as in the reference -- they run the same device kernels one phase at a
time (htm_sp_phase, include/bithtm_hip.h); an object that is not part of a SpatialPooler creates a small engine of
its own for that on first use."""

import numpy as np

from . import _lib as L


def checked_boosted(values, who):
    """Boosted overlaps on their way to the device's select (htm_sp_phase(HTM_SP_SELECT, data)) as contiguous float64.  The
    select orders every finite double >= 0, denormals and -0.0 (= 0) included; a NaN, an infinity or a negative value has no
    place in a top-k and is refused here, before anything runs on the device (the C entry point refuses them as well)."""
    x = np.ascontiguousarray(values, dtype=np.float64)
    bad = ~np.isfinite(x) | (x < 0)
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        raise ValueError(f"{who}: boosted overlaps must be finite and >= 0 (any double in [0, 1.8e308]); "
                         f"entry {i} is {x.reshape(-1)[i]!r}")
    return x


def checked_overlaps(values, who):
    """Overlaps on their way to the device's boosting (htm_sp_phase(HTM_SP_BOOST, data)) as contiguous int32: counts, so whole
    numbers in [0, 2^31).  Anything else is refused rather than truncated."""
    a = np.asarray(values)
    if a.dtype.kind not in "biu":
        with np.errstate(invalid="ignore"):
            whole = np.isfinite(a) & (a == np.rint(a)) if a.dtype.kind == "f" else None
        if whole is None or not whole.all():
            raise ValueError(f"{who}: overlaps must be whole numbers (counts of active connected inputs); got dtype {a.dtype}"
                             + ("" if whole is None else f", e.g. {a[~whole].reshape(-1)[0]!r}"))
    if a.size and (a.min() < 0 or a.max() > 2 ** 31 - 1):
        raise ValueError(f"{who}: overlaps must lie in [0, 2^31); got {a.min()!r} .. {a.max()!r}")
    return np.ascontiguousarray(a, dtype=np.int32)


def host_select_key(values):
    """NumPy twin of the key k_sp_keys gives a boosted overlap that came from the host (SP_KEYS_HOST, csrc/htm_sp_kernels.h): the
    double's bit pattern with the sign cleared.  Over finite doubles >= 0 it is strictly order-preserving, and -0.0 == +0.0."""
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)


class _Placeholder:
    """Parameters of a DenseProjection nobody evaluates (an engine needs some Spatial Pooler storage)."""

    def __init__(self, input_dim, output_dim):
        self.input_dim, self.output_dim = input_dim, output_dim
        self.permanence_threshold, self.permanence_increment, self.permanence_decrement = 0.0, 0.03, 0.015
        self._engine = None
        self._permanence = np.zeros((output_dim, input_dim), dtype=np.float64)


class ExponentialBoosting:
    """regularizations.py:4-21.  `duty_cycle` reads the float32 duty cycle from the device."""

    def __init__(self, output_dim, active_outputs, intensity=0.3, momentum=0.99):
        self.output_dim = output_dim
        self.active_outputs = active_outputs
        self.density = active_outputs / output_dim
        self.intensity = intensity
        self.momentum = momentum
        self._engine = None
        self._duty_cycle = np.zeros(output_dim, dtype=np.float32)

    @property
    def duty_cycle(self):
        if self._engine is not None:
            return self._engine.read_duty_cycle()
        return self._duty_cycle

    def _ensure_engine(self):
        if self._engine is None:
            from .engine import Engine
            eng = Engine(32, self.output_dim, 0, self.active_outputs, proximal=_Placeholder(32, self.output_dim), boosting=self)
            eng.write(L.F_DUTY_CYCLE, self._duty_cycle, np.float32)
            self._engine = eng
        return self._engine

    def process(self, input_activation):
        """regularizations.py:15-17 on the device: float32 factor (the documented exp), float64 product (one rounding, as
        NumPy's; exact while the overlap has at most 29 bits).  Overlaps are whole numbers in [0, 2^31)."""
        overlaps = checked_overlaps(input_activation, "ExponentialBoosting.process")
        eng = self._ensure_engine()
        eng.sp_phase(L.SP_BOOST, overlaps, np.int32)
        return eng.read(L.F_BOOSTED, np.float64, self.output_dim)

    def update(self, active_input):
        """regularizations.py:19-21 on the device (any order; a fancy-indexed += counts a repeated index once)."""
        eng = self._ensure_engine()
        eng.sp_phase(L.SP_ACTIVE, np.unique(np.asarray(active_input, dtype=np.int64).reshape(-1)), np.int32)
        eng.sp_phase(L.SP_DUTY)


class GlobalInhibition:
    """regularizations.py:24-29.  Selection is exact top-k with ties broken by lower column
    index; the winners are returned in ascending order.

    Accepted values: every finite float64 >= 0 -- denormals (from 5e-324), huge values (up to 1.8e308) and any mix of them
    in one array; -0.0 counts as 0.  All 64 bits of each value take part in the comparison: two values one ulp apart are
    not a tie.  NaN, +-inf and negative values raise ValueError (from the C entry point: HTM_ERR_ARGUMENT); the result is never
    a silently different list."""

    def __init__(self, active_outputs):
        self.active_outputs = active_outputs
        self._engine = None

    def process(self, input_activation):
        """regularizations.py:28-29 on the device (radix select of the k largest, ties to the lower index)."""
        x = checked_boosted(input_activation, "GlobalInhibition.process").reshape(-1)
        eng = self._engine
        if eng is None or eng.column_dim != len(x):
            from .engine import Engine
            eng = self._engine = Engine(32, len(x), 0, self.active_outputs, proximal=_Placeholder(32, len(x)),
                                        boosting=ExponentialBoosting(len(x), self.active_outputs))
        eng.sp_phase(L.SP_SELECT, x, np.float64)
        return eng.read(L.F_ACTIVE_COLUMN, np.int32, eng.active_columns).astype(np.int64)
