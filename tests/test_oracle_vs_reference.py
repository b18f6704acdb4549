"""Differential test: the unmodified reference (through its own hooks) vs. the oracle.

The reference's side is a recorded lock-step run (tests/golden/lockstep_*.npz, recorded by
tests/golden/generate_lockstep.py from a checkout of the reference, which checked every field of every step live while
recording): a digest of every output the reference returned each step and of its synapse store at the store checks.
Here the oracle runs the same inputs and must give every one of them."""

import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _replay(name):
    import refdiff
    rec = refdiff.load_lockstep(os.path.join(GOLDEN, f"lockstep_{name}.npz"))
    ora = refdiff.replay_lockstep(rec)
    assert ora.temporal_memory.S == int(rec["segments"])
    return ora, rec


def test_lockstep_small():
    ora, _ = _replay("small")
    assert ora.temporal_memory.S > 1000


def test_lockstep_with_a_wide_epsilon():
    """TemporalMemory.process(epsilon=0.3): best-matching and least-used ties a third of a count wide (several winner
    cells per bursting column, several best segments per cell)."""
    ora, rec = _replay("wide_epsilon")
    assert float(rec["epsilon"]) == pytest.approx(0.3)
    assert ora.temporal_memory.S > 500


def test_lockstep_with_earlier_states_as_prev_state():
    """TemporalMemory.process(prev_state=): every seventh step runs from the state of three steps earlier."""
    ora, rec = _replay("prev_state")
    assert [t for t in range(len(rec["back"])) if rec["back"][t] >= 0] == [t for t in range(11, 150) if t % 7 == 0]
    assert ora.temporal_memory.S > 500


def test_lockstep_learning_off_and_jumps():
    ora, rec = _replay("learning_off_jumps")
    assert [t for t in range(len(rec["learning"])) if not rec["learning"][t]] == [t for t in range(200) if t % 17 == 3]
    assert ora.temporal_memory.S > 500


def test_the_products_bridge_makes_the_reference_agree():
    """bithtm_amd.reference_bridge.keyed_rand -- what INTEGRATION.md hands to a maintainer of the reference -- in place of the
    test infrastructure's own patch: the unmodified reference, drawing the engine's keyed numbers through it, stays in
    lock-step with the oracle (and so with the engine, which the GPU tests pin to the oracle).  The run was recorded with the
    bridge; every call the reference made to it is replayed here from a stand-in with the caller's name and locals."""
    import refdiff
    from bithtm_amd.reference_bridge import keyed_rand, keyed_draws
    from oracle.keyed_rng import draw_unit
    ora, rec = _replay("bridge")
    assert ora.temporal_memory.S > 300
    # every draw the reference asked the bridge for, asked again: the same numbers
    arg_len, args = rec["call_arg_len"], rec["call_args"]
    ends = np.cumsum(arg_len)
    starts = ends - arg_len
    a = 0
    assert set(rec["call_where"].tolist()) == {0, 1, 2}
    with keyed_rand(int(rec["seed"]), int(rec["cell_dim"])) as patch:
        for i, (step, where, want) in enumerate(zip(rec["call_step"], rec["call_where"], rec["call_digest"])):
            where = refdiff.RAND_CALLERS[where]
            n = 2 if where == "add_edge" else 1
            call_args = [args[starts[j]:ends[j]] for j in range(a, a + n)]
            a += n
            shape = tuple(int(v) for v in rec["call_shape"][i][:rec["call_shape_len"][i]])
            patch.step = int(step)
            assert refdiff.digest(refdiff.call_rand_as(where, call_args, shape)) == want, f"call {i} ({where}, step {step})"
    assert a == len(arg_len)
    assert sum(patch.calls.values()) == len(rec["call_digest"])
    # ... and the C entry behind it gives the oracle's numbers
    a, b = np.arange(500, dtype=np.uint32) * 7919, np.arange(500, dtype=np.uint32)[::-1].copy()
    for stream in (1, 2, 3):
        assert np.array_equal(keyed_draws(35, stream, 99, a, b if stream == 2 else None), draw_unit(35, stream, 99, a, b if stream == 2 else 0))
