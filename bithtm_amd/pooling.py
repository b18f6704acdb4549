"""Pooling links of region stacks (include/bithtm_hip.h, htm_pool_columns): the definition, in NumPy over
integers.  The device path (csrc/htm_pool.h) is held to it bit for bit.

A plain link gives the upper level the OR of the lower level's active columns over a stride window.  A pooling link gives it a
decaying union instead: every lower column keeps a persistence P (uint8) that falls by `decay` per lower step and rises, when the
column is active, by `predicted_weight` if the lower level's last step predicted the column and by `active_weight` if not, up to
`ceiling`.  The upper level's input row has a bit for each of the `union_bits` columns of the largest persistence: a row that
stays put while the lower level is inside a sequence it knows, and differs from one sequence to another.

    P    = max(P - decay, 0)                                   # every column
    P[A] = min(ceiling, P[A] + where(prev[A], predicted_weight, active_weight))
    prev = colpred                                             # tm_state.cell_prediction.any(axis=1) of this step
    row  = bits of np.lexsort((arange(C), -P))[:union_bits] among the columns with P > 0      (at the end of a stride window)
"""

import numpy as np


class PoolingLink:
    """The parameters of a pooling link (RegionStack(links=[...])).  ValueError for anything outside
    stride >= 1, 0 <= active_weight, predicted_weight <= 255 (not both 0), 1 <= decay <= 255, 1 <= ceiling <= 255,
    union_bits None or >= 1 (None: min(lower column_dim, 2 * lower active_columns), resolved by the stack)."""

    PARAMETERS = ("stride", "active_weight", "predicted_weight", "decay", "ceiling", "union_bits")

    def __init__(self, stride=1, active_weight=1, predicted_weight=8, decay=1, ceiling=16, union_bits=None):
        values = dict(stride=stride, active_weight=active_weight, predicted_weight=predicted_weight, decay=decay, ceiling=ceiling)
        if union_bits is not None:
            values["union_bits"] = union_bits
        for name, v in values.items():
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"PoolingLink: {name} must be an integer (got {v!r})")
        self.stride, self.active_weight, self.predicted_weight = int(stride), int(active_weight), int(predicted_weight)
        self.decay, self.ceiling = int(decay), int(ceiling)
        self.union_bits = None if union_bits is None else int(union_bits)
        if self.stride < 1:
            raise ValueError(f"PoolingLink: stride >= 1 (got {stride})")
        if not (0 <= self.active_weight <= 255 and 0 <= self.predicted_weight <= 255) or self.active_weight == self.predicted_weight == 0:
            raise ValueError(f"PoolingLink: 0 <= active_weight, predicted_weight <= 255, not both 0 (got {active_weight}, {predicted_weight})")
        if not 1 <= self.decay <= 255:
            raise ValueError(f"PoolingLink: 1 <= decay <= 255 (got {decay})")
        if not 1 <= self.ceiling <= 255:
            raise ValueError(f"PoolingLink: 1 <= ceiling <= 255 (got {ceiling})")
        if self.union_bits is not None and self.union_bits < 1:
            raise ValueError(f"PoolingLink: union_bits >= 1 (got {union_bits})")

    def resolved(self, column_dim, active_columns):
        """This link over a lower level of `column_dim` columns with `active_columns` winners: union_bits filled in (None ->
        min(column_dim, 2 * active_columns)) and held to 1 <= union_bits <= column_dim (ValueError)."""
        bits = min(int(column_dim), 2 * int(active_columns)) if self.union_bits is None else self.union_bits
        if not 1 <= bits <= int(column_dim):
            raise ValueError(f"PoolingLink: 1 <= union_bits <= the lower level's column_dim {column_dim} (got {bits})")
        return PoolingLink(self.stride, self.active_weight, self.predicted_weight, self.decay, self.ceiling, bits)

    def as_array(self):
        """The six parameters as int64[6] in PARAMETERS' order (union_bits None: -1)."""
        return np.array([-1 if getattr(self, n) is None else getattr(self, n) for n in self.PARAMETERS], dtype=np.int64)

    def __eq__(self, other):
        return isinstance(other, PoolingLink) and self.as_array().tolist() == other.as_array().tolist()

    __hash__ = None

    def __repr__(self):
        return "PoolingLink(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.PARAMETERS) + ")"


class PoolingState:
    """The state of a pooling link over a lower level of C columns: `persistence` uint8[C] and `prev` bool[C] (the column
    prediction the lower level's last step left); both start at 0.  `link` is a resolved PoolingLink."""

    def __init__(self, link, column_dim):
        if link.union_bits is None:
            raise ValueError("PoolingState: the link's union_bits is not resolved (PoolingLink.resolved)")
        self.link, self.column_dim = link, int(column_dim)
        self.persistence = np.zeros(self.column_dim, dtype=np.uint8)
        self.prev = np.zeros(self.column_dim, dtype=np.bool_)

    def reset(self):
        """A sequence reset, before the step it precedes."""
        self.persistence[:] = 0
        self.prev[:] = False

    def step(self, active_column, column_prediction):
        """One lower step: its active columns (ids; one outside [0, C) counts for nothing) and its column prediction bool[C]."""
        lk = self.link
        P = np.maximum(self.persistence.astype(np.int64) - lk.decay, 0)
        A = np.asarray(active_column, dtype=np.int64).ravel()
        A = np.unique(A[(A >= 0) & (A < self.column_dim)])
        P[A] = np.minimum(lk.ceiling, P[A] + np.where(self.prev[A], lk.predicted_weight, lk.active_weight))
        self.persistence[:] = P
        self.prev[:] = np.asarray(column_prediction, dtype=np.bool_)

    def row(self):
        """The upper level's input row bool[C]: the union_bits columns of the largest persistence among those above 0, ties to
        the lower column index."""
        P = self.persistence.astype(np.int64)
        order = np.lexsort((np.arange(self.column_dim), -P))[:self.link.union_bits]
        out = np.zeros(self.column_dim, dtype=np.bool_)
        out[order[P[order] > 0]] = True
        return out
