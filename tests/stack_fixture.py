"""Shared by tests/test_region_stack_cpu.py and tests/test_hip_region_stack.py: the recorded two-level stack of the unmodified
reference (tests/golden/stack_two_level.npz, written by tests/golden/generate_stack.py), the chained oracles that replay it, and
the NumPy statement of htm_pack_columns' contract.  Not collected by pytest."""

import os
from types import SimpleNamespace

import numpy as np

import refdiff
from oracle import HTMOracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "stack_two_level.npz")
DIGESTS = ("active_column", "cell_prediction", "winner_cell")


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def inputs(fx):
    return refdiff.make_inputs(int(fx["seed"]) + 100, int(fx["patterns"]), int(fx["input_dim"]), float(fx["density"]))[0]


def schedule(fx):
    """learning[t], reset[t] per level-0 step of the recorded runs."""
    steps = int(fx["steps"])
    t = np.arange(steps)
    learning = ~((t >= fx["learning_off"][0]) & (t < fx["learning_off"][1]))
    return learning, np.isin(t, fx["resets"])


def initial_permanence(fx, level):
    """What the recorded reference of `level` drew: DenseProjection under np.random.seed(seed + level) (projections.py:16)."""
    dims = (int(fx["input_dim"]),) + tuple(int(c) for c in fx["column_dim"])
    np.random.seed(int(fx["seed"]) + level)
    return np.random.randn(dims[level + 1], dims[level]) * 0.1 + 0.0


def pack_columns(lists, input_dim, stride, bank, first_row):
    """htm_pack_columns in NumPy.  lists int[n_rows * stride, k]; bank uint32[bank_rows, W] (W = input_dim padded to 128 bits,
    in words), changed in place: row (first_row + r) % bank_rows = OR over the window's ids, pad bits 0; ids outside
    [0, input_dim) set nothing.  Returns whether such an id was met."""
    lists = np.asarray(lists, dtype=np.int64)
    n_rows = lists.shape[0] // stride
    bank_rows, W = bank.shape
    assert W == (input_dim + 127) // 128 * 4
    bad = False
    for r in range(n_rows):
        ids = lists[r * stride:(r + 1) * stride].ravel()
        ok = (ids >= 0) & (ids < input_dim)
        bad |= bool((~ok).any())
        bits = np.zeros(W * 32, dtype=np.bool_)
        bits[ids[ok]] = True
        bank[(first_row + r) % bank_rows] = np.packbits(bits, bitorder="little").view(np.uint32)
    return bad


def unpack_rows(bank, input_dim):
    return np.unpackbits(np.ascontiguousarray(bank).view(np.uint8), axis=1, bitorder="little")[:, :input_dim].astype(bool)


_EMPTY = {}


def _empty(C, K):
    if (C, K) not in _EMPTY:
        _EMPTY[(C, K)] = SimpleNamespace(cell_prediction=np.zeros((C, K), bool), cell_activation=np.zeros((C, K), bool), winner_cell=None,
                                         distal_state=None)
    return _EMPTY[(C, K)]


class OracleStack:
    """L chained oracles: the reference's loop of DESIGN.md section 14 (level l with seed + l)."""

    def __init__(self, input_dim, levels, strides, seed, permanences=None):
        self.levels, self.strides = [], list(strides)
        below = input_dim
        for l, (C, K, k) in enumerate(levels):
            if permanences is None:
                np.random.seed(seed + l)
            self.levels.append(HTMOracle(below, C, K, active_columns=k, seed=seed + l,
                                         permanence=None if permanences is None else permanences[l].copy()))
            below = C
        self.period = [1]
        for s in self.strides:
            self.period.append(self.period[-1] * s)
        self.window = [np.zeros(C, dtype=np.bool_) for C, _, _ in levels[:-1]]
        self.pending = [False] * len(levels)
        self.steps = 0
        self.upper_inputs = []                      # the input row of every step of level 1

    def reset(self):
        assert self.steps % self.period[-1] == 0
        self.pending = [True] * len(self.levels)

    def process(self, x, learning=True):
        out = [None] * len(self.levels)
        for l, ora in enumerate(self.levels):
            if self.pending[l]:
                sp = ora.spatial_pooler.step(x, learning=learning)
                tm = ora.temporal_memory.step(sp.active_column, learning=learning,
                                              prev_state=_empty(ora.temporal_memory.column_dim, ora.temporal_memory.cell_dim))
                self.pending[l] = False
            else:
                sp, tm = ora.step(x, learning=learning)
            out[l] = (sp, tm)
            if l + 1 == len(self.levels):
                break
            self.window[l][sp.active_column] = True
            if (self.steps + 1) % self.period[l + 1]:
                break
            x = self.window[l].copy()
            self.window[l][:] = False
            if l == 0:
                self.upper_inputs.append(x)
        self.steps += 1
        return out


def fixture_oracles(fx, stride):
    levels = [(int(C), int(K), int(k)) for C, K, k in zip(fx["column_dim"], fx["cell_dim"], fx["active_columns"])]
    return OracleStack(int(fx["input_dim"]), levels, [stride], int(fx["seed"]))


def state_digests(sp, tm, K):
    """The fixture's three digests of one level's step, from reference-shaped states."""
    return (refdiff.digest(sp.active_column), refdiff.digest(tm.cell_prediction),
            refdiff.digest(np.asarray(tm.winner_cell[0]) * K + np.asarray(tm.winner_cell[1])))


def check_step(fx, stride, level, index, sp, tm, segments):
    K = int(fx["cell_dim"][level])
    for name, got in zip(DIGESTS, state_digests(sp, tm, K)):
        assert got == fx[f"s{stride}_l{level}_{name}_digest"][index], f"stride {stride}, level {level}, step {index}: {name} differs from the reference's"
    assert segments == fx[f"s{stride}_l{level}_segments"][index], f"stride {stride}, level {level}, step {index}: segment count"
