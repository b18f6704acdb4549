"""The byte planes of the Spatial Pooler's connected mask (Dev::planes) and the overlap role of the two-launch schedule that
counts from them (role_overlap_planes): plane j holds, at byte c, byte j of column c's mask row; every kernel that writes the
mask keeps the planes exact, and a steady-state step of htm.run reads only the planes of the coming input's non-zero bytes.

The CPU test pins the indexing convention with a NumPy model.  The GPU tests run the smallest shapes at which the role can go
wrong against oracle.HTMOracle, every step's winners and each call's final state bit for bit, and end with
Engine.planes_check(): no plane byte differs from the mask, and the steps counted from the planes are the pipelined
steady-state steps the calls made (a call of n steps: n - 1, its last step looks at no coming input; a streamed call: n)."""

import copy

import numpy as np
import pytest

from oracle import HTMOracle, SPParams, TMParams

CAP = 1 << 16            # a fixed segment pool: one batch per run() call, so the steps of a call are the steps of one htm_run


# ---- the convention, on the CPU ------------------------------------------------------------------------------------------
def _pack(bits, words):
    """bit i -> bit (i & 31) of word (i >> 5), as the library packs inputs and mask rows"""
    padded = np.zeros(words * 32, dtype=np.uint8)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view("<u4")


def _planes_from_mask(mask):
    """mask: uint32 [C, W] -> planes uint8 [4 W, stride], stride = C rounded up to a multiple of 256"""
    C, W = mask.shape
    stride = (C + 255) & ~255
    planes = np.zeros((4 * W, stride), dtype=np.uint8)
    planes[:, :C] = np.ascontiguousarray(mask.astype("<u4")).view(np.uint8).reshape(C, 4 * W).T
    return planes


def _count_from_planes(planes, row, C):
    """what the role does: the non-zero bytes of the input row, and per column the bits its plane byte shares with each"""
    row_bytes = np.ascontiguousarray(row.astype("<u4")).view(np.uint8)
    cnt = np.zeros(C, dtype=np.int64)
    for j in np.flatnonzero(row_bytes):
        cnt += np.unpackbits((planes[j, :C] & row_bytes[j])[:, None], axis=1).sum(axis=1, dtype=np.int64)
    return cnt


@pytest.mark.parametrize("I,C", [(300, 70), (1000, 256), (2048, 300), (1, 5)])
def test_planes_model_equals_popcount_of_mask_and_input(I, C):
    W = (I + 127) // 128 * 4
    rng = np.random.RandomState(I + C)
    conn = rng.rand(C, I) < 0.4
    conn[0], conn[-1] = True, False
    mask = np.stack([_pack(r, W) for r in conn])
    planes = _planes_from_mask(mask)
    assert planes.shape == (4 * W, (C + 255) // 256 * 256)
    # the layout the header states: planes[j * stride + c] == byte j of column c's mask row
    for c, j in ((0, 0), (C - 1, 4 * W - 1), (C // 2, (I - 1) // 8)):
        assert planes[j, c] == (int(mask[c, j >> 2]) >> (8 * (j & 3))) & 0xFF
    assert not planes[(I + 7) // 8:].any() and not planes[:, C:].any()          # padding planes and padding columns stay zero
    rows = [rng.rand(I) < 0.03, np.zeros(I, bool), np.ones(I, bool), np.arange(I) == 0, np.arange(I) == I - 1, rng.rand(I) < 0.5]
    for x in rows:
        want = (conn & x).sum(axis=1)
        assert np.array_equal(_count_from_planes(planes, _pack(x, W), C), want)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------
def _pair(I, C, K, k, seed, cap=CAP):
    from hip_impl import make_htm
    np.random.seed(seed)
    ora = HTMOracle(I, C, K, active_columns=k, seed=seed)
    htm = make_htm(I, C, K, k, seed, ora.spatial_pooler.permanence.copy(), segment_capacity=cap)
    return ora, htm


def _compare_state(ora, htm, last, K):
    from hip_impl import compare_with_oracle, compare_store_with_oracle
    t = htm.engine.steps - 1
    h_sp = type(htm.spatial_pooler).State(htm.engine, htm.engine.steps)
    compare_with_oracle(t, last[0], last[1], h_sp, htm.temporal_memory.last_state, K)
    compare_store_with_oracle(t, ora, htm)


def _run(ora, htm, bank, n, K, learning=True, continuing=False, state=True):
    """n steps of htm.run beside the oracle: every step's winner list, and (state) everything the call leaves"""
    t0 = htm.engine.steps
    rec = htm.run(bank, n, learning=learning, continuing=continuing, record=("active_column",))
    last = None
    for i in range(n):
        last = ora.step(bank[(t0 + i) % len(bank)], learning=learning)
        assert np.array_equal(rec.active_column[i], last[0].active_column), f"step {t0 + i}: active columns"
    if state and not continuing:
        _compare_state(ora, htm, last, K)
    return last


def _bank(I, rows, density, seed):
    return np.random.RandomState(seed).rand(rows, I) < density


@pytest.mark.gpu
@pytest.mark.parametrize("I", [300, 1000, 2048])
def test_input_widths_from_scratch(I):
    """Ipad 384 (48 planes, 10 of them all padding, one partial), 1 024 and 2 048 (256 planes); 60 steps from scratch: the
    cold phase, tens of flipped mask bytes per winner row"""
    C, K, k = 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 21)
    bank = _bank(I, 7, 0.05, 22)
    _run(ora, htm, bank, 30, K)
    _run(ora, htm, bank, 30, K)
    assert htm.engine.planes_check() == (0, 58)


@pytest.mark.gpu
@pytest.mark.parametrize("C,k", [(2112, 42), (256, 8), (2304, 46)])
def test_column_counts(C, k):
    """a column count that is no multiple of the role's 256 columns per block (a partial last block), one block only, and a
    whole number of blocks"""
    I, K = 300, 8
    ora, htm = _pair(I, C, K, k, 31)
    bank = _bank(I, 6, 0.06, 32)
    _run(ora, htm, bank, 40, K)
    assert htm.engine.planes_check() == (0, 39)


def _adversarial(I, name):
    rng = np.random.RandomState(41)
    a, b, c = (rng.rand(I) < 0.05 for _ in range(3))
    if name == "zero_row":           # every overlap 0, one key: the tie goes to the lower index
        return np.stack([a, np.zeros(I, bool), b, c])
    if name == "ones_row":           # every plane is live
        return np.stack([a, np.ones(I, bool), b])
    if name == "single_bits":        # the first byte; the last valid bit of the last (partial) byte
        return np.stack([np.arange(I) == 0, a, np.arange(I) == I - 1, b])
    if name == "twice_running":      # the same columns win twice running: a row rewritten in consecutive launches
        return np.stack([a, a, b, b, c])
    raise KeyError(name)


@pytest.mark.gpu
@pytest.mark.parametrize("I,name", [(300, "zero_row"), (300, "ones_row"), (2048, "ones_row"), (300, "single_bits"),
                                    (1000, "single_bits"), (300, "twice_running")])
def test_adversarial_input_banks(I, name):
    C, K, k = 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 43)
    _run(ora, htm, _adversarial(I, name), 40, K)
    assert htm.engine.planes_check() == (0, 39)


@pytest.mark.gpu
def test_learning_off_then_on():
    """learning off: the role folds every column's duty cycle (fold 1), no row blocks; then on, in one stream"""
    I, C, K, k = 300, 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 51)
    bank = _bank(I, 5, 0.06, 52)
    _run(ora, htm, bank, 20, K, learning=False)
    _run(ora, htm, bank, 20, K, learning=True)
    assert htm.engine.planes_check() == (0, 38)


@pytest.mark.gpu
def test_other_writers_of_the_mask_in_between():
    """htm.run (streamed in chunks, with a one-step drain), host-fed steps, set_permanence on a row range, load_state_dict, and
    htm.run again: after each the planes equal the mask, and the next run equals the oracle"""
    from hip_impl import compare_with_oracle
    I, C, K, k = 300, 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 61)
    eng = htm.engine
    bank = _bank(I, 6, 0.06, 62)
    _run(ora, htm, bank, 9, K, continuing=True)
    _run(ora, htm, bank, 8, K, continuing=True)
    _run(ora, htm, bank, 1, K)                                      # the drain
    assert eng.planes_check() == (0, 17)
    saved, saved_ora = htm.state_dict(), copy.deepcopy(ora)
    for t in range(6):                                              # host-fed steps: the rows ride in other launches
        x = bank[(t * 5) % 6]
        o_sp, o_tm = ora.step(x)
        h_sp, h_tm = htm.process(x)
        compare_with_oracle(t, o_sp, o_tm, h_sp, h_tm, K)
    assert eng.planes_check() == (0, 17)
    _run(ora, htm, bank, 10, K)
    assert eng.planes_check() == (0, 26)
    rows = np.random.RandomState(63).randn(100, I) * 0.1 + 0.05     # rows 1 000..1 099 redrawn: a range that is no multiple of a tile
    eng.set_permanence(rows, 1000)
    ora.spatial_pooler.permanence[1000:1100] = rows
    assert eng.planes_check() == (0, 26)
    _run(ora, htm, bank, 10, K)
    assert eng.planes_check() == (0, 35)
    htm.load_state_dict(saved)
    ora = saved_ora
    assert htm.engine.planes_check()[0] == 0
    before = htm.engine.planes_check()[1]
    _run(ora, htm, bank, 10, K)
    assert htm.engine.planes_check() == (0, before + 9)


@pytest.mark.gpu
def test_stand_alone_pooler_learning_step_keeps_the_planes():
    """k_sp_learn, the learning launch of a stand-alone SpatialPooler (a handle of its own, unsharded: it keeps planes)"""
    import bithtm_amd as B
    from oracle import SpatialPoolerOracle
    I, C, k = 300, 1100, 22
    np.random.seed(71)
    ora = SpatialPoolerOracle(I, C, k)
    prox = B.DenseProjection(I, C)
    prox.permanence = ora.permanence.copy()
    sp = B.SpatialPooler(I, C, k, proximal_projection=prox)
    bank = _bank(I, 4, 0.08, 72)
    for t in range(12):
        want = ora.step(bank[t % 4], learning=t != 5)
        got = sp.process(bank[t % 4], learning=t != 5)
        assert np.array_equal(np.asarray(got.active_column), want.active_column), t
        assert np.array_equal(np.asarray(got.overlaps), want.overlaps), t
    assert np.array_equal(prox.permanence.view(np.int64), ora.permanence.view(np.int64))
    assert sp._engine.planes_check() == (0, 0)
    # ... and k_sp_run_tail, the learning launch of its batched run
    sp.run(bank, 9)
    for t in range(12, 21):
        ora.step(bank[t % 4])
    assert np.array_equal(prox.permanence.view(np.int64), ora.permanence.view(np.int64))
    assert sp._engine.planes_check() == (0, 0)


@pytest.mark.gpu
def test_three_launch_schedule_keeps_the_planes_it_does_not_read(monkeypatch):
    """BITHTM_LEAN=1: the rows ride in k_act_rows, which leaves the plane bytes to the launch behind it; the overlap stays
    column-major (no step is counted from the planes)"""
    monkeypatch.setenv("BITHTM_LEAN", "1")
    I, C, K, k = 300, 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 75)
    _run(ora, htm, _bank(I, 6, 0.06, 76), 30, K)
    assert htm.engine.planes_check() == (0, 0)


@pytest.mark.gpu
def test_a_view_counts_from_its_parents_planes():
    """an inference view's winners over a learned parent equal the oracle's Spatial Pooler with learning off (the view starts
    from the parent's duty cycles); the parent then learns 20 more steps and THE SAME view runs again: its winners are those of
    a pooler with the view's own duty cycles and the parent's new permanences -- the planes are the parent's, and current, not
    a copy made with the view"""
    I, C, K, k = 300, 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 81)
    bank = _bank(I, 5, 0.06, 82)
    probe = _bank(I, 7, 0.06, 83)
    _run(ora, htm, bank, 20, K)
    view = htm.inference_view()
    base = view.engine.planes_check()
    assert base[0] == 0
    frozen = copy.deepcopy(ora.spatial_pooler)
    changed = False
    for call in range(2):
        t0 = view.engine.steps
        rec = view.run(probe, 20, record=("active_column",))
        for i in range(20):
            want = frozen.step(probe[(t0 + i) % 7], learning=False)
            assert np.array_equal(rec.active_column[i], want.active_column), (call, i)
        assert view.engine.planes_check() == (0, base[1] + 19 * (call + 1))
        if call == 0:
            before = ora.spatial_pooler.permanence.copy()
            _run(ora, htm, bank, 20, K)
            connected = lambda perm: perm >= ora.spatial_pooler.params.permanence_threshold
            changed = bool((connected(before) != connected(ora.spatial_pooler.permanence)).any())
            frozen.permanence = ora.spatial_pooler.permanence.copy()       # the view's own duty cycles, the parent's new rows
    assert changed, "the parent's 20 steps changed no connected bit: the second pass would prove nothing"
    assert htm.engine.planes_check()[0] == 0


@pytest.mark.gpu
def test_four_launch_schedule_keeps_the_planes(monkeypatch):
    """BITHTM_LEAN=0: the rows ride in k_mid_rows one step ahead (role_sp_row with ahead = 1); no step counts from the planes"""
    monkeypatch.setenv("BITHTM_LEAN", "0")
    I, C, K, k = 300, 2048, 8, 41
    ora, htm = _pair(I, C, K, k, 85)
    _run(ora, htm, _bank(I, 6, 0.06, 86), 30, K)
    assert htm.engine.planes_check() == (0, 0)


@pytest.mark.gpu
def test_a_model_group_keeps_its_members_planes():
    """the group kernels rewrite each member's winner rows (role_sp_row in htm_group.h): after a group run every member's
    planes equal its mask, each member ends where its oracle does, and so does a member's own run() behind it"""
    import bithtm_amd as B
    I, C, K, k = 300, 2048, 8, 41
    pairs = [_pair(I, C, K, k, 87 + m) for m in range(2)]
    banks = [_bank(I, 5, 0.06, 90 + m) for m in range(2)]
    group = B.ModelGroup([htm for _, htm in pairs])
    group.run(banks, 20)
    for (ora, htm), bank in zip(pairs, banks):
        last = None
        for t in range(20):
            last = ora.step(bank[t % 5])
        _compare_state(ora, htm, last, K)
        assert htm.engine.planes_check() == (0, 0)
        _run(ora, htm, bank, 10, K)          # (two handles with streams of their own are live: this run is not pipelined)
        assert htm.engine.planes_check()[0] == 0


@pytest.mark.gpu
def test_a_sharded_handle_keeps_no_planes_and_runs_as_before():
    import bithtm_amd as B
    from bithtm_amd.distributed import LocalGroup
    I, C, K, seed = 256, 2048, 32, 91
    k = round(C * 0.02)
    np.random.seed(seed)
    perm = np.random.randn(C, I) * 0.1
    ora = HTMOracle(I, C, K, active_columns=k, seed=seed, permanence=perm)

    def parts(r):                                   # (as tests/test_hip_sharded.py builds a rank's parts)
        spp, tmp = SPParams(), TMParams()
        prox = B.DenseProjection.__new__(B.DenseProjection)
        prox.input_dim, prox.output_dim = I, C
        prox.permanence_threshold, prox.permanence_increment, prox.permanence_decrement = \
            spp.permanence_threshold, spp.permanence_increment, spp.permanence_decrement
        prox._engine, prox._permanence = None, perm
        return dict(proximal=prox, boosting=B.ExponentialBoosting(C, k, intensity=spp.boost_intensity, momentum=spp.boost_momentum),
                    distal=B.PredictiveProjection(C * K, **{f: getattr(tmp, f) for f in tmp.__dataclass_fields__}))
    group = LocalGroup(2, I, C, K, active_columns=k, make_parts=parts, seed=seed)
    bank = _bank(I, 5, 0.06, 92)
    from bithtm_amd import _lib as L
    for t in range(12):
        o_sp, _ = ora.step(bank[t % 5])
        group.process(bank[t % 5])
        for m in group.members:
            assert np.array_equal(m.engine.read(L.F_ACTIVE_COLUMN, np.int32, k), o_sp.active_column), (t, m.rank)
    for m in group.members:
        assert m.engine.planes_check() == (-1, 0)
