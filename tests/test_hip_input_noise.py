"""Device-side input noise (htm_bank_noise; HierarchicalTemporalMemory.run(noise=), InferenceView.run, ModelGroup.run; DESIGN.md
section 17): the fill kernel on its own against the NumPy definition (bithtm_amd.flip_noise) -- ring wrap, a source that does not
divide the window, the uint32 wrap of the step, sentinel rows, pad bits, reset words -- and noisy runs against a twin stepped
over the explicit host-built bank inputs[t % n] ^ flip_noise(seed, t, input_dim, p), one row per step: every record field and
the state left behind, bit for bit, in every schedule, across call and batch boundaries, through pool growth, against the
oracle; and that nothing else moved (graphs, the noise-free path)."""

import ctypes as C

import numpy as np
import pytest

from test_hip_run_record import ALL, SCHEDULES, SCHEDULE_IDS, _bank, _counters, _twins

SHAPE = (300, 1024, 8, 64)                          # the forecast fixture's small shape: input_dim, columns, cells, k
PATTERNS = 5
CHUNK = 7                                           # steps per fill: a 9-row ring that a 40-60 step run wraps several times


def _explicit(bank, first, n, seed, p):
    """Row t of the result = the input of step t for t in [first, first + n), zeros before: a twin whose step index is t reads
    it from a bank of first + n rows."""
    from bithtm_amd import flip_noise
    out = np.zeros((first + n, bank.shape[1]), bool)
    for t in range(first, first + n):
        out[t] = bank[t % len(bank)] ^ flip_noise(seed, t, bank.shape[1], p)
    return out


def _same_state(a, b, what=""):
    x, y = a.state_dict(), b.state_dict()
    assert x.keys() == y.keys()
    for key in x:
        assert np.array_equal(np.asarray(x[key]), np.asarray(y[key])), f"{what}: {key}"


def _same_record(got, want, what=""):
    assert len(got) == len(want), what
    assert np.array_equal(got.step_index, want.step_index), what
    bad = np.argwhere(_counters(got) != _counters(want))
    assert not len(bad), f"{what}: first (step, counter) mismatches {bad[:5].tolist()}"
    assert np.array_equal(got.active_column, want.active_column), what
    assert np.array_equal(got.column_prediction, want.column_prediction), what


# ---- the kernel alone

def _sp_engine(I):
    import bithtm_amd as B
    np.random.seed(1)
    return B.SpatialPooler(I, 64, 4)._ensure_engine()


def _peek(eng, ptr, words):
    eng.sync()
    out = np.empty(words, np.uint32)
    eng._hip_check(eng.lib.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2), "hipMemcpy")
    return out


def _poke(eng, ptr, words):
    eng.sync()
    words = np.ascontiguousarray(words, np.uint32)
    eng._hip_check(eng.lib.hipMemcpy(C.c_void_p(ptr), words.ctypes.data_as(C.c_void_p), words.nbytes, 1), "hipMemcpy")


def _pack(rows, W):
    out = np.zeros((len(rows), W * 4), np.uint8)
    pb = np.packbits(rows, axis=1, bitorder="little")
    out[:, :pb.shape[1]] = pb
    return out.view(np.uint32)


def _definition(src, flags, ring, bits, first, n_rows, seed, p):
    """The sequential loop of the definition on packed ring rows (uint32[n_dst, W]) and ring reset flags (all written)."""
    from bithtm_amd import flip_noise
    I, W, n_dst = src.shape[1], ring.shape[1], len(ring)
    ring, bits = ring.copy(), np.zeros_like(bits)
    for r in range(n_rows):
        step = (first + r) & 0xFFFFFFFF
        ring[step % n_dst] = _pack((src[step % len(src)] ^ flip_noise(seed, step, I, p))[None], W)[0]
        bits[step % n_dst] = flags[step % len(src)]
    return ring, bits


WINDOWS = [(7, 6), ((1 << 32) - 2, 5), (0, 9), (13, 1), (4, 0)]      # (first_step, n_rows) on a 9-row ring over 5 source rows


@pytest.mark.gpu
@pytest.mark.parametrize("I", [70, 300, 1000, 1024])
def test_bank_noise_equals_the_definition(I):
    """Engine.bank_noise + a raw read == the NumPy definition for p in {0, 0.05, 0.5, 1}: a window that wraps the ring (steps
    7..12 on 9 rows) over a source that does not divide it (5 rows), first_step = 2^32 - 2 with 5 rows (the step wraps for the
    noise and for the row index, and the steps 2^32 - 2 and 2 share ring row 2: the later one stays), a full ring, one row, no
    row.  The ring starts as all-ones sentinel words, pad words included: rows outside the window keep them, written rows have
    pad bits 0 (at p = 1 too); the reset word starts as all ones and comes out as the definition's, zeros outside the window."""
    from bithtm_amd import noise_threshold
    eng = _sp_engine(I)
    W, n_src, n_dst = eng.words, PATTERNS, CHUNK + 2
    assert W % 4 == 0 and W * 32 >= I
    rng = np.random.RandomState(I)
    src = rng.rand(n_src, I) < 0.3
    flags = np.array([1, 0, 0, 1, 0], bool)
    d_src, d_flags = eng.upload_bank(src), eng.upload_resets(flags)
    d_ring, d_bits = eng.zero_bank(n_dst), eng.zero_resets(n_dst)
    sentinel = np.full((n_dst, W), 0xFFFFFFFF, np.uint32)
    for p in (0.0, 0.05, 0.5, 1.0):
        for first, n_rows in WINDOWS:
            _poke(eng, d_ring, sentinel)
            _poke(eng, d_bits, np.full(1, 0xFFFFFFFF, np.uint32))
            eng.bank_noise(d_src, n_src, d_ring, n_dst, first, n_rows, 41, noise_threshold(p), d_flags, d_bits)
            want_ring, want_bits = _definition(src, flags, sentinel, np.zeros(n_dst, bool), first, n_rows, 41, p)
            got = _peek(eng, d_ring, n_dst * W).reshape(n_dst, W)
            assert np.array_equal(got, want_ring), (p, first, n_rows, np.flatnonzero((got != want_ring).any(axis=1)).tolist())
            assert np.array_equal(eng.read_resets(d_bits, n_dst), want_bits), (p, first, n_rows)
            assert _peek(eng, d_bits, 1)[0] >> n_dst == 0                   # (the word's bits above the ring's rows: 0)
            written = [((first + r) & 0xFFFFFFFF) % n_dst for r in range(n_rows)]
            for row in set(range(n_dst)) - set(written):
                assert (got[row] == 0xFFFFFFFF).all()                       # (sentinel rows: untouched)
            if p == 1.0 and n_rows:
                bits = np.unpackbits(got[written].view(np.uint8), axis=1, bitorder="little")
                assert not bits[:, I:].any() and bits[:, :I].sum(axis=1).min() > 0  # (pad bits 0 with every input flipped)
        # without reset pointers: the rows alone
        _poke(eng, d_ring, sentinel)
        eng.bank_noise(d_src, n_src, d_ring, n_dst, 7, 6, 41, noise_threshold(p))
        assert np.array_equal(_peek(eng, d_ring, n_dst * W).reshape(n_dst, W),
                              _definition(src, flags, sentinel, np.zeros(n_dst, bool), 7, 6, 41, p)[0])
    # read_bank sees the rows as run() will
    assert np.array_equal(eng.read_bank(d_ring, n_dst)[7], src[7 % n_src] ^ True)


@pytest.mark.gpu
def test_bank_noise_reset_words_of_a_ring_of_several_words():
    """A 70-row ring (three reset words, the last partly used) and a 37-row source with its own two words: every word is written
    whole -- the window's flags, zeros elsewhere -- for a window that wraps the ring and one across the uint32 wrap."""
    from bithtm_amd import noise_threshold
    I, n_src, n_dst = 300, 37, 70
    eng = _sp_engine(I)
    W = eng.words
    rng = np.random.RandomState(2)
    src, flags = rng.rand(n_src, I) < 0.2, rng.rand(n_src) < 0.4
    d_src, d_flags = eng.upload_bank(src), eng.upload_resets(flags)
    d_ring, d_bits = eng.zero_bank(n_dst), eng.zero_resets(n_dst)
    sentinel = np.full((n_dst, W), 0xFFFFFFFF, np.uint32)
    for first, n_rows in ((50, 40), ((1 << 32) - 30, 61), (3, 70)):
        _poke(eng, d_ring, sentinel)
        _poke(eng, d_bits, np.full(3, 0xFFFFFFFF, np.uint32))
        eng.bank_noise(d_src, n_src, d_ring, n_dst, first, n_rows, 3, noise_threshold(0.05), d_flags, d_bits)
        want_ring, want_bits = _definition(src, flags, sentinel, np.zeros(n_dst, bool), first, n_rows, 3, 0.05)
        assert np.array_equal(_peek(eng, d_ring, n_dst * W).reshape(n_dst, W), want_ring), (first, n_rows)
        assert np.array_equal(eng.read_resets(d_bits, n_dst), want_bits), (first, n_rows)
        assert want_bits.any() and _peek(eng, d_bits, 3)[2] >> (n_dst - 64) == 0


@pytest.mark.gpu
def test_bank_noise_refusals():
    from bithtm_amd import HtmError
    eng = _sp_engine(300)
    src, ring = eng.zero_bank(5), eng.zero_bank(9)
    flags, bits = eng.zero_resets(5), eng.zero_resets(9)
    for args in ((0, 5, ring, 9, 0, 1, 0, 0), (src, 5, 0, 9, 0, 1, 0, 0),              # null banks
                 (ring, 9, ring, 9, 0, 1, 0, 0),                                       # in place
                 (src, 5, ring, 9, 0, 10, 0, 0), (src, 5, ring, 9, 0, -1, 0, 0),       # n_rows outside [0, n_dst]
                 (src, 0, ring, 9, 0, 1, 0, 0), (src, 5, ring, 0, 0, 0, 0, 0),
                 (src, 5, ring, 9, 0, 1, 0, (1 << 24) + 1),                            # threshold above 2^24
                 (src, 5, ring, 9, 0, 1, 0, 0, flags, None), (src, 5, ring, 9, 0, 1, 0, 0, None, bits),
                 (src + 4, 5, ring, 9, 0, 1, 0, 0)):                                   # misaligned
        with pytest.raises(HtmError, match=r"\(-1\)"):
            eng.bank_noise(*args)
    eng.bank_noise(src, 5, ring, 9, 0, 9, 0, 1 << 24, flags, bits)                     # (the largest window and threshold)
    assert eng.read_bank(ring, 9).all()


# ---- noisy runs against the explicit bank

RESETS = np.array([1, 0, 0, 1, 0], bool)


@pytest.mark.gpu
@pytest.mark.parametrize("resets", [None, RESETS], ids=["no-resets", "resets"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "unpipelined"])
def test_noisy_run_equals_the_explicit_bank(pipeline, use_graph, resets):
    """run(noise=, noise_seed=) with noise_chunk = 7 == the twin over the explicit bank (one row per step, the reset flags tiled
    the same way): a recorded learning call, a call split with continuing=True on its first part, a call with learning off --
    every record and the state, bit for bit -- and a third model that takes the split call as one."""
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 3)
    p, seed, calls = 0.05, 77, ((23, True, False), (11, True, True), (17, True, False), (9, False, False))
    total = sum(n for n, _, _ in calls)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    one, _ = _twins(I, Cn, K, active_columns=k)
    htm.noise_chunk = one.noise_chunk = CHUNK
    explicit = _explicit(bank, 0, total, seed, p)
    assert (explicit != bank[np.arange(total) % PATTERNS]).any(axis=1).all()       # (every step's row is flipped somewhere)
    tiled = None if resets is None else resets[np.arange(total) % PATTERNS]
    for n, learning, continuing in calls:
        got = htm.run(bank, n, learning=learning, use_graph=use_graph, pipeline=pipeline, continuing=continuing, record=ALL,
                      resets=resets, noise=p, noise_seed=seed)
        want = twin.run(explicit, n, learning=learning, use_graph=use_graph, pipeline=pipeline, continuing=continuing, record=ALL,
                        resets=tiled)
        _same_record(got, want, f"call of {n}")
    _same_state(htm, twin, "split")
    # (the learning calls did learn: from the second step on every bursting column's winner cell grows a segment.  Whether the
    # model already predicts after these 51 noisy steps is a property of the model, not of the code under test: not asserted)
    assert int(htm.state_dict()["tm_S"]) > 0
    for n, learning in ((23, True), (28, True), (9, False)):
        one.run(bank, n, learning=learning, use_graph=use_graph, pipeline=pipeline, resets=resets, noise=p, noise_seed=seed)
    _same_state(one, htm, "a + b in one call")
    ring, bits, rows = htm._noise_rings[1][CHUNK + 2]
    assert rows == CHUNK + 2 and htm.engine.read_bank(ring, rows).shape == (CHUNK + 2, I)


@pytest.mark.gpu
@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
def test_streamed_noisy_chunks_in_every_schedule(env, monkeypatch):
    """run(continuing=True, noise=, resets=) in chunks, in every schedule the handle can take: the Spatial Pooler stays ahead
    across the calls -- one step in the two- and three-launch schedules, and the front of a second in the four-launch one --
    on rows the fill behind the call wrote and the next call's fill writes again."""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 7)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.noise_chunk = CHUNK
    chunks = (1, 2, 17, 7, 3, 26)
    total = sum(chunks)
    explicit, tiled = _explicit(bank, 0, total, 31, 0.05), RESETS[np.arange(total) % PATTERNS]
    for i, n in enumerate(chunks):
        got = htm.run(bank, n, continuing=i < 5, record=ALL, resets=RESETS, noise=0.05, noise_seed=31)
        want = twin.run(explicit, n, continuing=i < 5, record=ALL, resets=tiled)
        _same_record(got, want, f"chunk {i}")
    _same_state(htm, twin)


@pytest.mark.gpu
def test_default_seed_is_the_models_and_the_noise_matters():
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 3)
    htm, twin = _twins(I, Cn, K, seed=9, active_columns=k)
    plain, _ = _twins(I, Cn, K, seed=9, active_columns=k)
    htm.noise_chunk = CHUNK
    got = htm.run(bank, 40, record=ALL, noise=0.1)
    _same_record(got, twin.run(_explicit(bank, 0, 40, 9, 0.1), 40, record=ALL), "default seed")
    _same_state(htm, twin)
    assert not np.array_equal(got.active_column, plain.run(bank, 40, record=ALL).active_column)


@pytest.mark.gpu
def test_pool_growth_inside_a_noisy_run():
    """A default-sized pool that grows in the middle of run(noise=, resets=) (the shape and bank of the growth test of
    run(resets=)): the ring is made again on the new engine and the noise goes on with the step index."""
    I, Cn, K = 400, 1024, 8
    bank = _bank(500, I, 8, density=0.1)
    resets = np.zeros(500, bool)
    resets[::7] = True
    htm, twin = _twins(I, Cn, K)
    htm.noise_chunk = CHUNK
    first = htm.engine
    got = htm.run(bank, 500, record=ALL, resets=resets, noise=0.05, noise_seed=12)
    assert htm.engine is not first and htm._noise_rings[0]() is htm.engine      # (the pool did grow; the ring is the new engine's)
    want = twin.run(_explicit(bank, 0, 500, 12, 0.05), 500, record=ALL, resets=resets)
    _same_record(got, want, "growth")
    _same_state(htm, twin, "growth")


@pytest.mark.gpu
def test_noisy_run_equals_the_oracle():
    """The same run against the oracle stepped over the explicit rows: every step's active columns and column predictions
    from the record, and the store, duty cycles and permanences left behind."""
    from hip_impl import compare_store_with_oracle, make_htm
    from oracle import HTMOracle
    I, Cn, K, k = SHAPE
    steps, p, seed = 45, 0.05, 21
    np.random.seed(9)
    ora = HTMOracle(I, Cn, K, active_columns=k, seed=9, permanence=np.random.randn(Cn, I) * 0.1)
    htm = make_htm(I, Cn, K, k, 9, ora.spatial_pooler.permanence.copy())
    htm.noise_chunk = CHUNK
    bank = _bank(PATTERNS, I, 10)
    rec = htm.run(bank, steps, record=ALL, noise=p, noise_seed=seed)
    explicit = _explicit(bank, 0, steps, seed, p)
    for t in range(steps):
        o_sp, o_tm = ora.step(explicit[t])
        assert np.array_equal(rec.active_column[t], o_sp.active_column), t
        assert np.array_equal(rec.column_prediction[t], o_tm.cell_prediction.any(axis=1)), t
        assert rec.segments[t] == ora.temporal_memory.S, t
    compare_store_with_oracle(steps, ora, htm)


# ---- nothing else moved

@pytest.mark.gpu
def test_a_second_noisy_call_captures_no_new_graph():
    """The ring sits at one address: a second noisy call of the same length replays the graphs of the first (learning off
    after a learned stretch, so that nothing else a graph is keyed on -- the pool's size -- changes)."""
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 9)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.noise_chunk = CHUNK
    htm.run(bank, 60, noise=0.05)
    htm.run(bank, 40, learning=False, noise=0.05)
    n_graphs = htm.engine.graph_count()
    assert n_graphs > 0
    htm.run(bank, 40, learning=False, noise=0.05)
    assert htm.engine.graph_count() == n_graphs
    explicit = _explicit(bank, 0, 140, 5, 0.05)
    twin.run(explicit, 60)
    twin.run(explicit, 80, learning=False)
    _same_state(htm, twin)


@pytest.mark.gpu
def test_noise_and_then_none_leaves_nothing_behind():
    """A model that ran with noise (and reset flags) and then without ends as a twin that never took the argument: no reset
    bits, no ring, nothing of the noisy call stays with the handle."""
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 4)
    htm, twin = _twins(I, Cn, K, active_columns=k)
    htm.noise_chunk = CHUNK
    htm.run(bank, 33, noise=0.05, noise_seed=2, resets=RESETS)
    htm.run(bank, 41)
    twin.run(_explicit(bank, 0, 33, 2, 0.05), 33, resets=RESETS[np.arange(33) % PATTERNS])
    twin.run(bank, 41)
    _same_state(htm, twin)


@pytest.mark.gpu
def test_zero_noise_is_the_run_without_the_argument():
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 4)
    a, b = _twins(I, Cn, K, active_columns=k)
    ra = a.run(bank, 70, record=ALL, noise=0.0, noise_seed=3)
    rb = b.run(bank, 70, record=ALL)
    _same_record(ra, rb)
    _same_state(a, b)
    assert getattr(a, "_noise_rings", None) is None                             # (no ring was made)
    assert a.engine.graph_count() == b.engine.graph_count() and a.engine.device_bytes() == b.engine.device_bytes()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="noise"):
            a.run(bank, 5, noise=bad)
    with pytest.raises(ValueError, match="noise"):
        a.forecast(3, noise=0.05)
    _same_state(a, b)


# ---- views and groups

@pytest.mark.gpu
def test_view_run_with_noise_equals_the_view_over_the_explicit_bank():
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 3)
    parent, _ = _twins(I, Cn, K, active_columns=k)
    parent.run(bank, 60)
    view, twin = parent.inference_view(), parent.inference_view()
    view.noise_chunk = CHUNK
    first = view.engine.steps
    assert first == 60
    got = view.run(bank, 30, record=ALL, noise=0.05, noise_seed=11, resets=RESETS)
    explicit = _explicit(bank, first, 30, 11, 0.05)
    want = twin.run(explicit, 30, record=ALL, resets=RESETS[np.arange(first + 30) % PATTERNS])
    _same_record(got, want, "view")
    assert np.array_equal(view.predicted_input(), twin.predicted_input())
    with pytest.raises(ValueError, match="learning"):
        view.run(bank, 5, learning=True, noise=0.05)


@pytest.mark.gpu
def test_group_run_with_noise_equals_each_member_alone():
    """ModelGroup.run(noise=[...], noise_seed=[...]) == every member run alone with its own values (one member without noise);
    and with default seeds two members on the same rows read different rows -- each its own seed's."""
    import bithtm_amd as B
    from bithtm_amd import flip_noise
    I, Cn, K, k = SHAPE
    bank = _bank(PATTERNS, I, 3)
    seeds, ps, noise_seeds = [1, 2, 3], [0.05, 0.0, 0.2], [7, 8, 9]
    np.random.seed(4)
    group = B.ModelGroup.create(3, I, Cn, K, seeds=seeds, active_columns=k)
    np.random.seed(4)
    solo = [B.HierarchicalTemporalMemory(I, Cn, K, active_columns=k, seed=s) for s in seeds]
    group.noise_chunk = CHUNK
    inputs = np.stack([bank] * 3)
    recs = group.run(inputs, 40, record=ALL, noise=ps, noise_seed=noise_seeds)
    for i, m in enumerate(solo):
        m.noise_chunk = CHUNK
        _same_record(recs[i], m.run(bank, 40, record=ALL, noise=ps[i], noise_seed=noise_seeds[i]), f"member {i}")
        _same_state(group.models[i], m, f"member {i}")
    # one probability for all, default seeds: each member's own
    recs = group.run(inputs, 20, record=ALL, noise=0.05)
    rows = []
    for i, m in enumerate(group.models):
        ring, _, n = m._noise_rings[1][CHUNK + 2]
        rows.append(m.engine.read_bank(ring, n))
        last = m.engine.steps - 1                                               # (the last step's row is still in the ring)
        assert np.array_equal(rows[i][last % n], bank[last % PATTERNS] ^ flip_noise(seeds[i], last, I, 0.05)), i
    assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])
    for i, m in enumerate(solo):
        _same_record(recs[i], m.run(bank, 20, record=ALL, noise=0.05), f"member {i}, default seed")
    with pytest.raises(ValueError, match="noise"):
        group.run(inputs, 5, noise=[0.1, 0.2])
    with pytest.raises(ValueError, match="noise_seed"):
        group.run(inputs, 5, noise=0.1, noise_seed=[1, 2])
