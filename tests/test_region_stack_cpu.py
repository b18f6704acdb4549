"""Region stacks without a GPU: the chained oracles against the recorded two-level stack of the unmodified reference
(tests/golden/generate_stack.py), the NumPy statement of htm_pack_columns' contract against the recorded upper-level inputs,
the C ABI of htm_pack_columns (declared, exported, argument checks that need no device) and the refusals of RegionStack that
can be decided without a device."""

import os
import re

import numpy as np
import pytest

import stack_fixture as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return sf.load()


@pytest.fixture(scope="module")
def replays(fx):
    """The chained oracles through both recorded runs, every digest checked on the way -> {stride: OracleStack}."""
    import refdiff
    bank = sf.inputs(fx)
    learning, reset = sf.schedule(fx)
    out = {}
    for stride in fx["strides"].tolist():
        ora = sf.fixture_oracles(fx, stride)
        for l, o in enumerate(ora.levels):
            assert refdiff.digest(o.spatial_pooler.permanence) == fx[f"s{stride}_permanence_digest"][l]
        upper = 0
        for t in range(int(fx["steps"])):
            if reset[t]:
                ora.reset()
            res = ora.process(bank[t % len(bank)], learning=bool(learning[t]))
            sf.check_step(fx, stride, 0, t, *res[0], ora.levels[0].temporal_memory.S)
            if res[1] is not None:
                assert refdiff.digest(ora.upper_inputs[-1]) == fx[f"s{stride}_upper_input_digest"][upper]
                sf.check_step(fx, stride, 1, upper, *res[1], ora.levels[1].temporal_memory.S)
                upper += 1
            else:
                assert (t + 1) % stride
        assert upper == int(fx["steps"]) // stride == len(fx[f"s{stride}_l1_segments"])
        out[stride] = ora
    return out


def test_chained_oracles_replay_the_reference_at_both_levels_and_strides(fx, replays):
    assert sorted(replays) == [1, 3]
    learning, reset = sf.schedule(fx)
    assert (~learning).sum() >= 8 and reset.sum() >= 3                 # a learning-off stretch, a few resets ...
    assert all(int(r) % 3 == 0 for r in fx["resets"])                  # ... on window boundaries of both runs


def test_the_fixture_pins_the_upper_temporal_memory(fx):
    """At the top level more than half of the steps after the first two passes through the patterns predict a column (the
    reference's own predictions, as recorded): otherwise the upper level's digests would say nothing about its Temporal Memory."""
    patterns = int(fx["patterns"])
    for stride in fx["strides"].tolist():
        later = fx[f"s{stride}_l1_predicted"][-(-2 * patterns // stride):]
        assert later.size > 40 and later.mean() > 0.5, (stride, later.mean())
        assert fx[f"s{stride}_l1_segments"][-1] > 100


def test_pack_contract_reproduces_the_recorded_upper_inputs(fx):
    """OR over windows, rotation by first_row, zero pad bits: the NumPy statement of htm_pack_columns, fed with level 0's
    recorded lists, gives the rows the reference's upper level was fed."""
    import refdiff
    C0 = int(fx["column_dim"][0])
    W = (C0 + 127) // 128 * 4
    for stride in fx["strides"].tolist():
        lists = fx[f"s{stride}_l0_lists"].astype(np.int64)
        want = fx[f"s{stride}_upper_input_digest"]
        n = len(want)
        for bank_rows, first_row in ((n, 0), (n, 7), (n + 5, n - 2)):
            bank = np.full((bank_rows, W), 0xDEADBEEF, dtype=np.uint32)
            assert not sf.pack_columns(lists, C0, stride, bank, first_row)
            rows = sf.unpack_rows(bank, C0)
            for r in range(n):
                assert refdiff.digest(rows[(first_row + r) % bank_rows]) == want[r], (stride, bank_rows, first_row, r)
            written = {(first_row + r) % bank_rows for r in range(n)}
            for r in set(range(bank_rows)) - written:
                assert (bank[r] == 0xDEADBEEF).all()
    # pad bits are zero, and an id outside the range sets nothing and is reported
    bank = np.full((2, 4), 0xFFFFFFFF, dtype=np.uint32)
    assert sf.pack_columns(np.array([[0, 99, 100], [5, -1, 31]]), 100, 1, bank, 1)
    assert bank[1].tolist() == [1, 0, 0, 8] and bank[0].tolist() == [(1 << 5) | (1 << 31), 0, 0, 0]


def test_header_declares_and_library_exports_pack_columns():
    from bithtm_amd import _lib
    header = open(os.path.join(ROOT, "include", "bithtm_hip.h")).read()
    assert re.search(r"int htm_pack_columns\(htm_handle \*dst, const int32_t \*device_lists, int32_t k, int32_t n_rows, int32_t stride,\s*"
                     r"uint32_t \*device_bank, int32_t bank_rows, int32_t first_row\);", header)
    assert "#define BITHTM_ABI_VERSION 4" in header
    assert "htm_pack_columns" in _lib.EXPORTS
    lib = _lib.load()
    assert lib.htm_abi_version() == _lib.ABI_VERSION == 4
    assert lib.htm_pack_columns is not None


def test_pack_columns_rejects_null_arguments_without_a_device():
    import ctypes as C
    from bithtm_amd import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * 4)()
    assert lib.htm_pack_columns(None, None, 1, 1, 1, None, 1, 0) == -1
    assert lib.htm_pack_columns(None, C.cast(buf, C.c_void_p), 1, 1, 1, C.cast(buf, C.c_void_p), 1, 0) == -1


def test_region_stack_is_exported_and_refuses_what_needs_no_device():
    import bithtm_amd as B
    from bithtm_amd import RegionStack
    assert RegionStack is B.stack.RegionStack
    for name in ("of", "process", "run", "reset", "state_dict", "load_state_dict", "save", "load"):
        assert callable(getattr(RegionStack, name))
    assert "not the fast path" in RegionStack.process.__doc__
    # the constructor: malformed levels and strides, cell_dim above 64 -- all before anything touches a device
    for levels, strides in (([], None), ([(64,)], None), ([(64, 4, 2, 1)], None), ([(64, 4), (32, 4)], [1, 1]), ([(64, 4), (32, 4)], [0]),
                            ([(64, 4), (32, 4)], []), ([(64, 65)], None), ([(64, 4), (32, 70)], None), ([(64, 4, 65)], None)):
        with pytest.raises(ValueError):
            RegionStack(10, levels, strides=strides)
    with pytest.raises(ValueError):
        RegionStack(0, [(64, 4)])
    # of(): models whose Temporal Memory steps on the host (cell_dim above 64: no engine is made for them)
    a, b, c = B.HierarchicalTemporalMemory(10, 64, 65), B.HierarchicalTemporalMemory(64, 32, 65), B.HierarchicalTemporalMemory(48, 32, 65)
    assert a.engine is None
    with pytest.raises(ValueError, match="column_dim"):
        RegionStack.of([a, c])                      # the dims do not chain
    with pytest.raises(ValueError, match="cell_dim"):
        RegionStack.of([a, b])
    with pytest.raises(ValueError):
        RegionStack.of([])
    with pytest.raises(ValueError):
        RegionStack.of([a, b], strides=[1, 2])
    with pytest.raises(ValueError):
        RegionStack.of([object()])

    class Layer:                                    # plug-in objects on the host
        def process(self, x, learning=True):
            return None
    host = B.HierarchicalTemporalMemory(10, 64, 4, spatial_pooler=Layer(), temporal_memory=Layer())
    with pytest.raises(ValueError, match="host"):
        RegionStack.of([host])
