"""Plug-ins that make the *unmodified* reference deterministic.  TEST INFRASTRUCTURE ONLY.

The reference exposes constructor hooks (`networks.py:16,22-24`: `boosting=`,
`inhibition=`) and draws its random numbers from the module-global `np.random.rand`.
This file supplies

  * `StableTopK`       -- an `inhibition=` object (interface of GlobalInhibition,
                          regularizations.py:24-29) implementing the documented tie rule;
  * `DocumentedExpBoosting` -- a `boosting=` object (interface of ExponentialBoosting,
                          regularizations.py:4-21) whose only difference is the exp;
  * `keyed_rand(...)`  -- a context manager replacing `np.random.rand` by the keyed
                          generator.  The replacement looks at its caller's frame to learn
                          what the draw is for (which cells / segments), because the
                          reference only passes a shape.

None of this is imported by the product.  It needs the reference on sys.path only for the
frame's function names; it contains no reference code.
"""

import contextlib
import os
import sys

import numpy as np

from .fexp import exp_f32
from .htm_oracle import stable_topk, sp_derived, SPParams
from .keyed_rng import draw_unit, STREAM_LEAST_USED, STREAM_GROWTH, STREAM_SEGMENT_JITTER


class StableTopK:
    def __init__(self, active_outputs):
        self.active_outputs = active_outputs
        self.ambiguous_calls = 0
        self.calls = 0

    def process(self, input_activation):
        from .htm_oracle import topk_is_unambiguous
        self.calls += 1
        if not topk_is_unambiguous(input_activation, self.active_outputs):
            self.ambiguous_calls += 1
        return stable_topk(input_activation, self.active_outputs)


class DocumentedExpBoosting:
    def __init__(self, output_dim, active_outputs, intensity=0.3, momentum=0.99):
        self.density = active_outputs / output_dim
        self.intensity = intensity
        self.momentum = momentum
        self.duty_cycle = np.zeros(output_dim, dtype=np.float32)
        self._d = sp_derived(SPParams(boost_intensity=intensity, boost_momentum=momentum),
                             output_dim, active_outputs)

    def process(self, input_activation):
        factor = exp_f32(self._d.coef32 * self.duty_cycle)
        return factor * input_activation

    def update(self, active_input):
        self.duty_cycle *= self.momentum
        self.duty_cycle[active_input] += 1.0 - self.momentum


class KeyedRand:
    """Callable standing in for np.random.rand while the reference runs one TM step."""

    def __init__(self, seed, cell_dim, fallback):
        self.seed = seed
        self.cell_dim = cell_dim
        self.step = 0
        self.fallback = fallback
        self.log = []          # (step, stream, shape) of every keyed draw
        self.growth_ties = 0   # rows where a priority tie straddled the growth cut (counted in the add_edge branch below)

    def __call__(self, *shape):
        frame = sys._getframe(1)
        name = frame.f_code.co_name
        loc = frame.f_locals
        if name == "evaluate_cell_least_used":            # networks.py:87
            cols = np.asarray(loc["relevant_column"], dtype=np.int64)
            flat = cols[:, None] * self.cell_dim + np.arange(self.cell_dim)
            out = draw_unit(self.seed, STREAM_LEAST_USED, self.step, flat)
            stream = STREAM_LEAST_USED
        elif name == "add_edge":                           # projections.py:120
            segs = np.asarray(loc["learning_output"], dtype=np.int64)
            winners = np.asarray(loc["winner_input"], dtype=np.int64)
            out = np.zeros((len(segs), len(winners) + 1), dtype=np.float64)
            if len(segs) and len(winners):
                out[:, :-1] = draw_unit(self.seed, STREAM_GROWTH, self.step, segs[:, None], winners[None, :])
                # a tie between the last priority taken and the first one left out (projections.py:124-127 sorts with an
                # unstable argsort: which of the two grows is implementation-defined; the oracle takes the lower winner index)
                n_add = np.asarray(loc["added_output_edges"], dtype=np.int64).reshape(-1)
                pri = out[:, :-1].astype(np.float32)
                at = np.asarray(loc["whole_input_to_winner"])[np.asarray(loc["learning_edge_target"])]
                rows, cols = np.nonzero(at < len(winners))
                pri[rows, at[rows, cols]] = np.inf                                     # :121 (already connected)
                pri.sort(axis=1)
                cut = np.flatnonzero((n_add > 0) & (n_add < len(winners)))
                last, first_out = pri[cut, n_add[cut] - 1], pri[cut, n_add[cut]]
                self.growth_ties += int(((last == first_out) & np.isfinite(last)).sum())
            stream = STREAM_GROWTH
        elif name == "fill_jittered_potential_info":       # projections.py:235
            segs = np.asarray(loc["state"].matching_segment, dtype=np.int64)
            out = draw_unit(self.seed, STREAM_SEGMENT_JITTER, self.step, segs)
            stream = STREAM_SEGMENT_JITTER
        else:
            return self.fallback(*shape)
        assert out.shape == tuple(shape), (name, out.shape, shape)
        self.log.append((self.step, stream, tuple(shape)))
        return out


@contextlib.contextmanager
def keyed_rand(seed, cell_dim):
    original = np.random.rand
    patch = KeyedRand(seed, cell_dim, original)
    np.random.rand = patch
    try:
        yield patch
    finally:
        np.random.rand = original


def import_reference(path=None):
    """Import the reference package read-only from a checkout of cokwa/bitHTM: `path`, or the directory the environment
    variable BITHTM_REFERENCE names (only the scripts that record tests/golden/ need it)."""
    path = path or os.environ.get("BITHTM_REFERENCE")
    if not path or not os.path.isdir(os.path.join(path, "bithtm")):
        raise RuntimeError("set BITHTM_REFERENCE to a checkout of the reference (cokwa/bitHTM): the directory that holds bithtm/")
    if path not in sys.path:
        sys.path.insert(0, path)
    import bithtm  # noqa: F401
    from bithtm import networks, projections, regularizations, reference_implementations
    return SimpleNamespaceLike(bithtm=bithtm, networks=networks, projections=projections,
                               regularizations=regularizations,
                               reference_implementations=reference_implementations)


class SimpleNamespaceLike:
    def __init__(self, **kw):
        self.__dict__.update(kw)
