"""Closed-loop forecasting in reference terms, shared by tests/golden/generate_forecast.py (which runs the unmodified reference
beside the oracle), tests/test_forecast_cpu.py and tests/test_hip_forecast.py.  Not collected by pytest.

    votes  = (pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0)
    x      = encode(votes, min_votes, max_bits)
    process(x, learning=False)
"""

import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forecast.npz")

RUN = dict(seed=37, input_dim=300, column_dim=1024, cell_dim=8, active_columns=64, patterns=8, density=0.06, epochs=40, context=2,
           steps=20)
CASES = [(8, 18), (1, 10), (2, 0)]                  # (min_votes, max_bits): two that sustain the sequence, one whose rows go empty


def votes_of(permanence, threshold, cell_prediction):
    """(pp.permanence[tm_state.cell_prediction.any(axis=1)] >= pp.permanence_threshold).sum(axis=0)"""
    return (permanence[np.asarray(cell_prediction).any(axis=1)] >= threshold).sum(axis=0).astype(np.int32)


def encode(votes, min_votes, max_bits):
    """The issue's definition, verbatim: most votes first, ties to the LOWER input index."""
    assert min_votes >= 1 and max_bits >= 0
    votes = np.asarray(votes)
    I = votes.size
    x = votes >= min_votes
    if max_bits and x.sum() > max_bits:
        keep = np.lexsort((np.arange(I), -votes.astype(np.int64)))[:max_bits]
        x = np.zeros(I, bool)
        x[keep] = True
    return x


def pack_rows(rows):
    """bool[n, I] -> uint8[n, ceil(I / 8)], bit i of a row = bit (i & 7) of byte (i >> 3)."""
    return np.packbits(np.asarray(rows, dtype=bool), axis=1, bitorder="little")


def unpack_rows(packed, input_dim):
    return np.unpackbits(packed, axis=1, bitorder="little")[:, :input_dim].astype(bool)


def training_inputs(cfg):
    """The bank of the run, and the rows of its training and context steps in order (the bank cycled)."""
    bank = np.random.RandomState(int(cfg["seed"]) + 1).rand(int(cfg["patterns"]), int(cfg["input_dim"])) < float(cfg["density"])
    n_train = int(cfg["patterns"]) * int(cfg["epochs"])
    return bank, n_train, n_train + int(cfg["context"])


def trained_oracle(cfg):
    """The oracle after the training steps (learning on) and the context steps (learning off)."""
    from oracle import HTMOracle
    seed, I, C, K, k = (int(cfg[f]) for f in ("seed", "input_dim", "column_dim", "cell_dim", "active_columns"))
    np.random.seed(seed)
    ora = HTMOracle(I, C, K, active_columns=k, seed=seed)
    bank, n_train, n_all = training_inputs(cfg)
    tm = None
    for t in range(n_all):
        _, tm = ora.step(bank[t % len(bank)], learning=t < n_train)
    return ora, tm


def oracle_closed_loop(ora, tm, steps, min_votes, max_bits):
    """`steps` closed-loop steps of the oracle from the state `tm` left: (rows bool[steps, I], votes int32[steps, I] of the state
    each step leaves, active columns int32[steps, k])."""
    sp_o = ora.spatial_pooler
    rows, votes_after, cols = [], [], []
    for _ in range(steps):
        x = encode(votes_of(sp_o.permanence, sp_o.params.permanence_threshold, tm.cell_prediction), min_votes, max_bits)
        sp, tm = ora.step(x, learning=False)
        rows.append(x)
        votes_after.append(votes_of(sp_o.permanence, sp_o.params.permanence_threshold, tm.cell_prediction))
        cols.append(np.sort(np.asarray(sp.active_column)))
    return np.asarray(rows, bool), np.asarray(votes_after, np.int32), np.asarray(cols, np.int32)
