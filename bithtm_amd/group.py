"""Model groups: many independent models of one shape stepped together (htm_group_*, include/bithtm_hip.h; DESIGN.md
section 11).

HTM's common use is one model per data stream.  One model at a small shape (the reference's 1 000 inputs -> 2 048 columns x 32
cells) leaves the GPU idle between its launches; a group steps B members with ONE launch sequence, every launch covering all
of them, and every member ends bit-identical to the same model stepped alone.

    group = ModelGroup.create(64, input_dim=1000, column_dim=2048, cell_dim=32, seeds=range(64))
    group.run(inputs, steps)                  # inputs: bool [64, n_inputs, 1000]; member i cycles through inputs[i]
    rec = group.process(x)                    # x: bool [64, 1000], one tick of every member; rec.anomaly_score[i]
    group.models[3].process(x[3])             # members stay ordinary models between group calls

    views = ModelGroup.views(trained, 16)     # 16 inference views of one trained model: one copy of the weights, and the
    views.run(inputs, steps)                  # store scanned once per step for up to M of them together (learning=False)
"""

import ctypes as C

import numpy as np

from . import _lib as L
from .engine import CapacityError, HtmError, pack_bits
from .networks import (RECORD_COUNTERS, HierarchicalTemporalMemory, InferenceView, RunRecord, _BatchedCall, _batches, _cached_bank, _check_encoder,
                       _encode_params, _no_classifier, _no_knn, _noise_ring, _record_fields, _with_counters, noise_threshold, retire_states)
from .knn_classifier import KNNClassifierBank
from .sdr_classifier import SDRClassifierBank, model_shape


class SharedStream:
    """A HIP stream of the library's runtime that several engines enqueue on (HierarchicalTemporalMemory(stream=...)); the
    engines keep it alive, and it is destroyed after the last of them."""

    def __init__(self, device=0):
        self.lib = L.load()
        out = C.c_void_p()
        rc = self.lib.hipSetDevice(int(device))
        if rc == 0:
            rc = self.lib.hipStreamCreateWithFlags(C.byref(out), 1)       # hipStreamNonBlocking
        if rc != 0:
            raise HtmError(f"hipStreamCreateWithFlags failed ({rc}): {self.lib.hipGetErrorString(rc).decode()}")
        self.handle = out.value

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self.lib.hipStreamDestroy(h)


class GroupTick(RunRecord):
    """What ModelGroup.tick() returns: row i is member i's step of this tick.  RunRecord's counters and derived properties
    (correct_columns, incorrect_columns, anomaly_score), step_index int64 [B], and
      capacity_error    int32 [B]   each member's sticky capacity flags after the step (engine.info().capacity_error)
      predicted_bucket, predicted_score int32 [B, F], predicted_value float64 [B, F]   with an encoder: the votes of the state
                                    the step leaves, decoded per field on the device; NaN where nothing is predicted
      predicted_input   int32 [B, input_dim]   with predicted_input=True: those votes themselves
      anomaly_likelihood float64 [B]  with likelihood=: each member's anomaly likelihood of this step (log_likelihood: its log scale)
      classified_bucket int32 [B, H], classified_probability float64 [B, H]   with classifier=: per horizon of the SDRClassifierBank
                                    each member's most probable bucket and its probability; classified_value float64 [B, H] for a
                                    bank of an encoder field; class_distribution int32 [B, H, buckets] with class_distribution=True
      knn_label, knn_votes, knn_overlap, knn_nearest_slot, knn_nearest_step int32 [B]   with knn=: each member's result row of the
                                    KNNClassifierBank (knn.ROW); knn_votes_all int32 [B, labels] with knn_votes_all=True"""

    def __init__(self, rows, pairs=None, votes=None, encoder=None, anomaly_likelihood=None, classified=None, class_distribution=None,
                 classified_field=None, knn=None, knn_votes_all=None):
        counters = np.stack([rows[name] for name in RECORD_COUNTERS], axis=1)
        bucket = score = value = None
        if pairs is not None:
            bucket, score = np.ascontiguousarray(pairs[:, :, 0]), np.ascontiguousarray(pairs[:, :, 1])
            value = encoder.value_of(bucket)
        super().__init__(rows["step_index"], counters=counters, predicted_input=votes, predicted_bucket=bucket, predicted_score=score,
                         predicted_value=value, anomaly_likelihood=anomaly_likelihood, classified=classified,
                         class_distribution=class_distribution, classified_field=classified_field, knn=knn, knn_votes_all=knn_votes_all)
        self.capacity_error = np.ascontiguousarray(rows["capacity_error"], dtype=np.int32)


_CAPACITY_FLAGS = ((1, "segment pool (segment_capacity)"), (2, "synapse slots (segment_slots)"), (4, "work list / growth staging"),
                   (8, "dead-segment report (DEAD_CAP)"))


def _refuse_member(i, m):
    """Why model i cannot be a group member (ValueError), or None."""
    if not isinstance(m, HierarchicalTemporalMemory):
        return f"member {i} is a {type(m).__name__}, not a HierarchicalTemporalMemory (column-sharded models cannot join a group)"
    if not getattr(m.temporal_memory, "_own_distal", False) and getattr(m.temporal_memory, "cell_dim", 0) > 64:
        return f"member {i} has cell_dim {m.cell_dim} > 64: its Temporal Memory steps on the host"
    if m.engine is None:
        return f"member {i} has a layer or a distal projection that lives on the host (plug-in objects)"
    if not m.spatial_pooler._plain:
        return f"member {i} has plug-in Spatial Pooler objects that run on the host"
    if m._streaming:
        return f"member {i} is in the middle of a streamed run() (continuing=True): end the stream first"
    return None


class ModelGroup:
    """B fused HierarchicalTemporalMemory models of one shape (input_dim, column_dim, cell_dim <= 64, active_columns, segment
    pool), stepped by one launch sequence.  Seeds, learning parameters and learned state may differ.  The members stay
    ordinary models: process(), run(), state_dict() and the rest work on them between group calls."""

    def __init__(self, models):
        models = list(models)
        if not models:
            raise ValueError("a model group needs at least one member")
        for i, m in enumerate(models):
            why = _refuse_member(i, m)
            if why:
                raise ValueError(why)
        for i, m in enumerate(models):
            for j in range(i):
                if models[j] is m:
                    raise ValueError(f"member {i} is member {j} again")
        e0 = models[0].engine
        for i, m in enumerate(models):
            e = m.engine
            for attr in ("input_dim", "column_dim", "cell_dim", "active_columns", "segment_capacity", "segment_slots"):
                if getattr(e, attr) != getattr(e0, attr):
                    raise ValueError(f"member {i}: {attr} {getattr(e, attr)} differs from member 0's {getattr(e0, attr)}")
            if not self._has_views(models) and e._auto_grow != e0._auto_grow:
                raise ValueError(f"member {i}: either every member's segment pool is default-sized (and grows) or none is")
        self.models = models
        self.lib = L.load()
        self._g = None
        self._engines = None
        self._auto_grow = e0._auto_grow and not self._has_views(models)     # (views never add a segment: nothing to look at)
        self._build()

    @staticmethod
    def _has_views(models):
        return any(isinstance(m, InferenceView) for m in models)

    @classmethod
    def views(cls, parent, n, fork=False):
        """A group of n inference views of `parent` (parent.inference_view() n times): n input streams over one copy of its
        weights, stepped with learning=False.  The views' scan reads the shared segment store once per step for up to M of
        them at a time (M: as many members' column bitmaps as fit 64 KiB of LDS, at most 16).  `fork=True`: every member is
        parent.fork() -- it continues the parent's stream from where that is now (one launch per member) instead of starting
        as after reset()."""
        if n < 1:
            raise ValueError("ModelGroup.views: n must be at least 1")
        return cls([parent.fork() if fork else parent.inference_view() for _ in range(int(n))])

    def _learning(self, learning):
        """learning=None: False for a group with inference views, True for any other (as before); True with views: ValueError."""
        views = self._has_views(self.models)
        if learning is None:
            return not views
        if learning and views:
            raise ValueError("a group with inference views steps with learning=False only (its views share their parent's weights)")
        return bool(learning)

    @classmethod
    def create(cls, n, input_dim, column_dim, cell_dim, seeds=None, active_columns=None, device=0, **kw):
        """n members with seeds `seeds` (default 0 .. n-1) on ONE shared stream (so each member keeps the fastest schedule in
        its own solo calls, and the group needs no events to join them).  Further keywords go to HierarchicalTemporalMemory."""
        seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
        if len(seeds) != n:
            raise ValueError(f"seeds: {n} values, got {len(seeds)}")
        stream = SharedStream(device)
        return cls([HierarchicalTemporalMemory(input_dim, column_dim, cell_dim, active_columns=active_columns, seed=s, device=device,
                                               stream=stream, **kw) for s in seeds])

    def __len__(self):
        return len(self.models)

    def __del__(self):
        self._destroy()

    def _destroy(self):
        g, self._g = getattr(self, "_g", None), None
        if g:
            self.lib.htm_group_destroy(g)

    def _build(self):
        """The C group over the members' current engines (again after any of them was re-created: grow_pool)."""
        self._destroy()
        engines = [m.engine for m in self.models]
        handles = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
        out = C.c_void_p()
        rc = self.lib.htm_group_create(handles, len(engines), C.byref(out))
        if rc != 0:
            raise HtmError(f"htm_group_create failed ({rc}): {self.lib.htm_group_last_error(None).decode()}")
        self._g, self._engines = out, engines

    def _check(self, rc, what):
        if rc < 0:
            raise HtmError(f"{what} failed ({rc}): {self.lib.htm_group_last_error(self._g).decode()}")

    def _current(self):
        for i, m in enumerate(self.models):
            if m._streaming:
                raise ValueError(f"member {i} is in the middle of a streamed run() (continuing=True): end the stream first")
        for m in self.models:
            if isinstance(m, InferenceView):
                m._check_parent()
        if self._g is None or any(m.engine is not e for m, e in zip(self.models, self._engines)):
            self._build()

    def _grow(self, per_step, force_check):
        """Pool growth of default-sized pools, for all members alike: if any member needs more room, every member grows to the
        largest capacity and slot count any of them asks for (the shapes stay equal).  True if the members were re-created."""
        engines = [m.engine for m in self.models]
        wanted = [e._grow_to for e in engines if e.pool_look(per_step, force=force_check)]
        if not wanted:
            return False
        cap = max([engines[0].segment_capacity] + [c for c, _ in wanted if c])
        slots = max([engines[0].segment_slots] + [s for _, s in wanted if s])
        self._destroy()                             # (before the old engines go)
        for m in self.models:
            m.grow_pool(cap, slots)
        self._build()
        return True

    def _records(self, fields, n, encoder=None):
        """Per member: the record buffers of n steps (the members' own, as run(record=) uses) -> (HtmRunRecord array -- None when
        only "predicted_input" / "predicted_value" are asked for -- and each member's {field: device address}, which
        _read_records takes).  "predicted_input": each member's decoding rows are set (_unset_votes clears them);
        "predicted_value" (with `encoder`) uses the same rows."""
        recs = (L.HtmRunRecord * len(self.models))()
        buffers = [m.engine._record_args(fields, n, recs[i], encoder) for i, m in enumerate(self.models)]
        return (None if not set(fields) - {"predicted_input", "predicted_value"} else recs), buffers

    def _unset_votes(self):
        for m in self.models:
            m.engine.set_run_predicted_input(None)

    def _read_records(self, fields, n, buffers, encoder=None):
        """`buffers`: what _records returned for this call."""
        if encoder is not None:                 # (behind the group's launches: on the same stream, or -- members on streams of
            for m, member in zip(self.models, buffers):             # their own -- behind the wait that ends such a call)
                m.engine.decode_records(member, n, encoder)
        for m in self.models:                   # (the group enqueues on the first member's stream)
            m.engine.sync()
        return [m.engine._records_read(fields, n, encoder=encoder) for m in self.models]

    def _banks(self, inputs, encoder=None):
        """Each member's device bank of its rows of `inputs`, uploaded once and cached as run() caches it."""
        ptrs = [_cached_bank(m, m.engine, x, encoder=encoder) for m, x in zip(self.models, inputs)]
        return (C.c_void_p * len(ptrs))(*ptrs)

    def _bank_targets(self, bank, targets, inputs, encoder, what):
        """run() / tick() with classifier=: the members' target buckets -> int32 [B, rows] (tick: rows = 1).  `inputs`: the members'
        rows [B, rows, ...]; None `targets` with an encoder and a bank made with field=: encoder.bucket of the field, on the host."""
        B = len(self.models)
        if targets is None:
            if encoder is None or bank.field is None:
                raise ValueError(f"{what}(classifier=): give targets=, or encoder= and a bank made with field=")
            where = [j for j, f in enumerate(encoder.fields) if f is bank.field]
            if not where:
                raise ValueError(f"{what}(classifier=): the bank's field is not one of the encoder's fields")
            targets = np.stack([encoder.bucket(inputs[i])[:, where[0]] for i in range(B)])
        targets = np.asarray(targets)
        if targets.ndim != 2 or targets.shape != (B, inputs.shape[1]):
            raise ValueError(f"targets: int [{B}, {inputs.shape[1]}], one bucket per member and row, got {list(targets.shape)}")
        return bank.check_targets(targets)

    # run(noise=): steps per fill of the members' noise rings (see HierarchicalTemporalMemory.noise_chunk)
    noise_chunk = 1024

    def run(self, inputs, steps, learning=None, use_graph=True, record=None, resets=None, noise=0.0, noise_seed=None, encoder=None,
            likelihood=None, classifier=None, targets=None, classifier_learning=None, knn=None, labels=None, knn_learning=None):
        """`steps` timesteps of every member, member i over the rows of inputs[i] (bool [B, n_inputs, input_dim]), cycled, as
        its own run(inputs[i], steps) would.  Returns None, or (`record`: as run(record=)) one RunRecord per member.
        learning=None: True, or False in a group with inference views (which refuses True).
        `noise`, `noise_seed`: as run(noise=, noise_seed=), one value or one per member; member i then ends as its own
        run(inputs[i], steps, noise=noise[i], noise_seed=noise_seed[i]) would.  The default seed is each member's own, so members
        on the same rows still see different noise.  With all of them 0 the call is the one without noise.
        `encoder`: as run(encoder=), one ScalarEncoder for all members: `inputs` is then float64 [B, n_inputs, F], each member's
        values, encoded on the device into its bank, and `record` may name "predicted_value".
        `likelihood`: an AnomalyLikelihood of B streams -- the call records the counters (as record=True), behind each batch ONE
        htm_likelihood_update runs over the members' record buffers (a table of B pointers, never a launch per member) before the
        read-back, and member i's RunRecord.anomaly_likelihood is stream i's.
        `classifier`: an SDRClassifierBank of B streams (a one-stream SDRClassifier is refused) -- the call records the counters,
        every step leaves every member's active-cell words on the device (htm_set_group_run_active_cells: one small launch per
        step for all members, set for this call only), and behind each batch ONE htm_classifiers_update runs over the members'
        patterns before the read-back, never a launch sequence per member.  `targets`: int [B, n_inputs], the bucket of each
        member's rows (-1: missing), uploaded once; None with `encoder`: the bucket of the bank's field among the encoder's.  With
        `noise`, targets index the row of `inputs`.  `classifier_learning`: None follows `learning`.  Member i's RunRecord gains
        classified_bucket, _probability, _value and (with "class_distribution" named in `record`) class_distribution, as
        run(classifier=) of the member alone with stream i as its classifier would give them.
        `knn`: a KNNClassifierBank of B streams (a one-stream KNNClassifier is refused; over views: KNNClassifierBank.shared) -- it
        rides on the call as the classifier bank does, over the same captured words (with both, the steps' patterns are captured
        once), and behind each batch ONE htm_knns_update runs over every member's patterns.  `labels`: int [B, n_inputs], the label
        of each member's rows (-1, or anything outside [0, knn.labels): none), rolled per member as the targets are and uploaded
        once; None: nothing is labelled.  `knn_learning`: None follows `learning`.  ValueError before anything is enqueued when any
        stream's labelled steps do not fit its store.  Member i's RunRecord gains knn_label, knn_votes, knn_overlap,
        knn_nearest_slot, knn_nearest_step and (with "knn_votes_all" named in `record`) knn_votes_all, as run(knn=) of the member
        alone with stream i as its KNNClassifier would give them."""
        near = knn if isinstance(knn, KNNClassifierBank) else None
        if near is None:
            _no_knn(knn, "ModelGroup.run()")
        bank = classifier if isinstance(classifier, SDRClassifierBank) else None
        if bank is None:
            _no_classifier(classifier, "ModelGroup.run()")
        learning = self._learning(learning)
        B = len(self.models)
        cls_learn = distribution = False
        if bank is not None:
            if bank.streams != B:
                raise ValueError(f"run(classifier=): an SDRClassifierBank of {B} streams, got {bank.streams}")
            cls_learn = bool(learning if classifier_learning is None else classifier_learning)
            bank._no_shared_learning(cls_learn)
            names = () if record is None or record is True else ((record,) if isinstance(record, str) else tuple(record))
            distribution = "class_distribution" in names
            if distribution:
                record = tuple(f for f in names if f != "class_distribution") or None
            record = _with_counters(record)
        elif targets is not None or classifier_learning is not None:
            raise ValueError("run(): targets= and classifier_learning= go with classifier=")
        knn_learn = votes_all = False
        if near is not None:
            if near.streams != B:
                raise ValueError(f"run(knn=): a KNNClassifierBank of {B} streams, got {near.streams}")
            knn_learn = bool(learning if knn_learning is None else knn_learning)
            near._no_shared_learning(knn_learn)
            names = () if record is None or record is True else ((record,) if isinstance(record, str) else tuple(record))
            votes_all = "knn_votes_all" in names
            if votes_all:
                record = tuple(f for f in names if f != "knn_votes_all") or None
            record = _with_counters(record)
        elif labels is not None or knn_learning is not None:
            raise ValueError("run(): labels= and knn_learning= go with knn=")
        if likelihood is not None:
            if likelihood.streams != B:
                raise ValueError(f"run(likelihood=): an AnomalyLikelihood of {B} streams, got {likelihood.streams}")
            record = _with_counters(record)
        if np.ndim(noise) > 1 or (np.ndim(noise) == 1 and len(noise) != B):
            raise ValueError(f"noise: one probability or one per member ({B}), got shape {np.shape(noise)}")
        thresholds = [noise_threshold(p) for p in np.broadcast_to(np.asarray(noise, dtype=np.float64), (B,))]
        seeds = [None] * B
        if noise_seed is not None:
            if np.ndim(noise_seed) > 1 or (np.ndim(noise_seed) == 1 and len(noise_seed) != B):
                raise ValueError(f"noise_seed: one seed or one per member ({B}), got shape {np.shape(noise_seed)}")
            seeds = [int(x) for x in np.broadcast_to(np.asarray(noise_seed, dtype=np.int64), (B,))]
        if resets is not None:
            raise NotImplementedError("sequence resets inside a group run are not available yet (the follow-up: k_tm_reset per "
                                      "member inside the group's launches); reset members with model.reset() between group calls")
        fields = None if record is None else _record_fields(record)
        e0 = self.models[0].engine
        _check_encoder(encoder, fields, e0.input_dim, e0.column_dim)
        if encoder is None:
            inputs = np.asarray(inputs, dtype=np.bool_)
            if inputs.ndim != 3 or inputs.shape[0] != B or inputs.shape[2] != e0.input_dim:
                raise ValueError(f"inputs: bool [{B}, n_inputs, {e0.input_dim}], got {inputs.shape}")
        else:
            inputs = np.ascontiguousarray(inputs, dtype=np.float64)
            if inputs.ndim != 3 or inputs.shape[0] != B or inputs.shape[1] < 1 or inputs.shape[2] != len(encoder):
                raise ValueError(f"inputs: float64 values [{B}, n_inputs, {len(encoder)}], got {inputs.shape}")
        host_targets = None
        if bank is not None:
            bank._set_shape(*model_shape(e0))
            host_targets = self._bank_targets(bank, targets, inputs, encoder, "run")
        host_labels = None
        if near is not None:
            near._set_shape(*model_shape(e0))
            host_labels = near.check_labels(np.full((B, inputs.shape[1]), -1) if labels is None else labels)
            if host_labels.shape != (B, inputs.shape[1]):
                raise ValueError(f"labels: int [{B}, {inputs.shape[1]}], one label per member and row, got {list(host_labels.shape)}")
        for m in self.models:
            retire_states(m.engine)
        self._current()
        k = self.models[0].active_columns
        if near is not None:
            # member i's labels rolled by its distance from member 0's step, so that one first_step serves all members; the whole
            # call's room is looked at before its first batch
            e0, rows_in = self.models[0].engine, inputs.shape[1]
            host_labels = np.stack([np.roll(g, -((m.engine.steps - e0.steps) % rows_in)) for g, m in zip(host_labels, self.models)])
            near.check_room(near.stored_by(host_labels, e0.steps % rows_in, int(steps), knn_learn))
        call = _BatchedCall([m.temporal_memory for m in self.models], fields, encoder, likelihood is not None, bank, near)
        device_targets = device_labels = None

        def pools():        # cut into batches the smallest free-segment budget of any member lasts, with a look at the pools between them
            while self._grow(2 * k, True):
                pass
            return [(min(m.engine._free_segments for m in self.models), 2 * k, 1)]
        for _, n in _batches(steps, pools if self._auto_grow else None, cap=int(self.noise_chunk) if any(thresholds) else None):
            banks, n_inputs = self._banks(inputs, encoder), inputs.shape[1]
            if any(thresholds):
                # each member's ring filled for the steps of this batch and the one behind it (members without noise: a copy of
                # their rows), then the group over the rings -- the order forecast() uses for its seed rows
                n_inputs = int(self.noise_chunk) + 2
                rings = []
                for m, src, thr, seed in zip(self.models, banks, thresholds, seeds):
                    e = m.engine
                    if e.steps + n + 1 > 1 << 32:
                        raise ValueError("run(noise=): the run would pass step 2^32, where the device's step counter wraps")
                    ring, ring_resets, _ = _noise_ring(m, e, self.noise_chunk)
                    e.bank_noise(src, inputs.shape[1], ring, n_inputs, e.steps, n + 1, e.seed if seed is None else seed, thr,
                                 e.upload_resets(np.zeros(inputs.shape[1], dtype=np.bool_)), ring_resets)
                    rings.append(ring)
                banks = (C.c_void_p * B)(*rings)
            if fields is None:
                self._check(self.lib.htm_group_run(self._g, banks, n_inputs, n, int(bool(learning)), int(bool(use_graph)), None),
                            "htm_group_run")
            else:
                recs, buffers = self._records(fields, n, encoder)
                if near is not None and bank is None:       # (with a classifier bank as well: its capture below serves both)
                    e0, rows_in, per = self.models[0].engine, inputs.shape[1], near.shape[2]
                    cells = near.pairs_buffer(e0, n)
                    cell_rows = [cells + i * n * per * 8 for i in range(B)]
                    self._check(self.lib.htm_set_group_run_active_cells(self._g, (C.c_void_p * B)(*cell_rows)), "htm_set_group_run_active_cells")
                if near is not None and knn_learn and device_labels is None:
                    device_labels = near.upload_labels(self.models[0].engine, host_labels)
                if bank is not None:
                    # every member's rows of this batch in one buffer [B][n][pairs]; the targets by the row of `inputs` a step reads:
                    # member i's rolled by its distance from member 0's step, so that one first_step serves all members
                    e0, rows_in, per = self.models[0].engine, inputs.shape[1], bank.shape[2]
                    cells = bank.pairs_buffer(e0, n)
                    cell_rows = [cells + i * n * per * 8 for i in range(B)]
                    if device_targets is None:
                        rolled = np.stack([np.roll(t, -((m.engine.steps - e0.steps) % rows_in)) for t, m in zip(host_targets, self.models)])
                        device_targets = bank.upload_targets(e0, rolled)
                    self._check(self.lib.htm_set_group_run_active_cells(self._g, (C.c_void_p * B)(*cell_rows)), "htm_set_group_run_active_cells")
                try:
                    self._check(self.lib.htm_group_run(self._g, banks, n_inputs, n, int(bool(learning)), int(bool(use_graph)), recs),
                                "htm_group_run")
                finally:
                    self._unset_votes()
                    if bank is not None or near is not None:
                        self.lib.htm_set_group_run_active_cells(self._g, None)
                if likelihood is not None:          # (on the group's stream -- the first member's -- behind the run, before the wait)
                    likelihood.enqueue(self.models[0].engine, [b["counters"] for b in buffers], n)
                if bank is not None:                # (likewise: ONE update over every member's patterns)
                    bank.enqueue(e0, cell_rows, per, n, [device_targets + i * rows_in * 4 for i in range(B)], rows_in, e0.steps % rows_in, None, cls_learn,
                                 distribution)
                if near is not None:                # (likewise, over the same captured words)
                    near.enqueue(e0, cell_rows, per, n, device_labels, host_labels if knn_learn else None, e0.steps % rows_in, knn_learn, votes_all)
                parts = self._read_records(fields, n, buffers, encoder)
                if near is not None:
                    rows5, votes = near.read(e0, n, votes_all)
                    for i, part in enumerate(parts):
                        part["knn"], part["knn_votes_all"] = rows5[i].copy(), (votes[i].copy() if votes is not None else None)
                if bank is not None:
                    best, dist = bank.read(e0, n, distribution)
                    for i, part in enumerate(parts):
                        part["classified"], part["class_distribution"] = best[i].copy(), (dist[i].copy() if dist is not None else None)
                if likelihood is not None:
                    for part, row in zip(parts, likelihood.read(self.models[0].engine, n)):
                        part["anomaly_likelihood"] = row
                call.add(parts)
            for m in self.models:
                m.engine.steps += n
        for m in self.models:
            m._streaming = False
        records = call.finish([steps] * B, [k] * B)
        return None if fields is None else records

    def run_into(self, banks, n_inputs, n_steps, buffers, learning=None, use_graph=True):
        """The group's counterpart of Engine.run_into -- a run of every member, enqueued only: member i over the `n_inputs` rows of
        the device bank banks[i], its records into buffers[i] = {record field: device address of its n_steps rows} (empty
        dictionaries: a plain htm_group_run).  Nothing is synchronised, nothing is read back, no pool is looked at: the caller
        orders its own work behind the group's stream (stacks of groups feed "active_column" to htm_group_pack_columns)."""
        learning = self._learning(learning)
        B, n = len(self.models), int(n_steps)
        if len(banks) != B or len(buffers) != B:
            raise ValueError(f"run_into(): {B} banks and {B} buffer dictionaries, one per member")
        for m in self.models:
            retire_states(m.engine)
        self._current()
        recs = (L.HtmRunRecord * B)()
        votes = [m.engine._record_ptrs(b, recs[i]) for i, (m, b) in enumerate(zip(self.models, buffers))]
        recorded = any(set(b) - {"predicted_input", "predicted_value"} for b in buffers)
        try:
            for m, v in zip(self.models, votes):
                if v is not None:
                    m.engine.set_run_predicted_input(v)
            self._check(self.lib.htm_group_run(self._g, (C.c_void_p * B)(*banks), int(n_inputs), n, int(bool(learning)), int(bool(use_graph)),
                                               recs if recorded else None), "htm_group_run")
        finally:
            if any(v is not None for v in votes):
                self._unset_votes()
        for m in self.models:
            m.engine.steps += n
            m._streaming = False

    def _link_tables(self, lists, banks, first_rows):
        B = len(self.models)
        if not (len(lists) == len(banks) == len(first_rows) == B):
            raise ValueError(f"{B} lists, banks and first rows, one per member")
        return (C.c_void_p * B)(*lists), (C.c_void_p * B)(*banks), (C.c_int32 * B)(*[int(r) for r in first_rows])

    def pack_columns(self, lists, k, n_rows, stride, banks, bank_rows, first_rows):
        """Bank rows of every member from recorded active-column lists (htm_group_pack_columns: Engine.pack_columns of member i
        with the i-th entries, in ONE launch): enqueued on the group's stream, no wait."""
        self._current()
        lists, banks, first = self._link_tables(lists, banks, first_rows)
        self._check(self.lib.htm_group_pack_columns(self._g, lists, int(k), int(n_rows), int(stride), banks, int(bank_rows), first), "htm_group_pack_columns")

    def pool_columns(self, link, lists, k, column_predictions, n_rows, persistences, prevs, reset_bits, scratch, scratch_bytes, banks, bank_rows, first_rows):
        """Bank rows of every member through a pooling link (htm_group_pool_columns: Engine.pool_columns of member i with the i-th
        entries, three launches per batch whatever B is; `reset_bits`: None, or one address or None per member): enqueued on the
        group's stream, no wait."""
        self._current()
        B = len(self.models)
        lists, banks, first = self._link_tables(lists, banks, first_rows)
        if not (len(column_predictions) == len(persistences) == len(prevs) == B) or (reset_bits is not None and len(reset_bits) != B):
            raise ValueError(f"{B} column predictions, persistences, prevs and reset bits, one per member")
        p = L.HtmPoolLink(C.sizeof(L.HtmPoolLink), link.stride, link.active_weight, link.predicted_weight, link.decay, link.ceiling, link.union_bits, 0)
        table = lambda ptrs: (C.c_void_p * B)(*ptrs)
        self._check(self.lib.htm_group_pool_columns(self._g, p, lists, int(k), table(column_predictions), int(n_rows), table(persistences), table(prevs),
                                                    None if reset_bits is None else table(reset_bits), C.c_void_p(scratch), int(scratch_bytes), banks,
                                                    int(bank_rows), first), "htm_group_pool_columns")

    # forecast(): steps per feeding group run (see HierarchicalTemporalMemory.forecast_chunk)
    forecast_chunk = 1024

    def forecast(self, steps, min_votes=1, max_bits=0, record=None, use_graph=True, encoder=None):
        """Every member's forecast(steps, min_votes, max_bits) at once: each member rolls forward from its own state on its own
        encoded votes, one launch sequence per step for all members.  min_votes / max_bits: one value, or one per member.
        Returns bool [B, steps, input_dim]; with `record` (as run(record=)) the pair (rows, one RunRecord per member).  `encoder`:
        the ScalarEncoder a "predicted_value" record decodes with."""
        B, steps = len(self.models), int(steps)
        params = [_encode_params(a, b) for a, b in zip(np.broadcast_to(np.asarray(min_votes), (B,)), np.broadcast_to(np.asarray(max_bits), (B,)))]
        fields = None if record is None else _record_fields(record)
        _check_encoder(encoder, fields, self.models[0].engine.input_dim, self.models[0].engine.column_dim)
        engines = [m._forecast_engine("forecast()") for m in self.models]
        for e in engines:
            retire_states(e)
        self._current()
        engines = [m.engine for m in self.models]
        chunk, k = int(self.forecast_chunk), self.models[0].active_columns
        ptrs = [m._zero_bank(e, chunk + 1) for m, e in zip(self.models, engines)]
        banks = (C.c_void_p * B)(*ptrs)
        rows = np.zeros((B, steps, engines[0].input_dim), dtype=np.bool_)
        call = _BatchedCall([m.temporal_memory for m in self.models], fields, encoder)
        for done, n in _batches(steps, cap=chunk):
            start = [e.steps for e in engines]
            recs = None
            try:
                for e, ptr, (mv, mb) in zip(engines, ptrs, params):
                    e.encode_votes(mv, mb, ptr, chunk + 1, e.steps % (chunk + 1))
                    e.set_run_feedback(ptr, chunk + 1, mv, mb)
                if fields is not None:
                    recs, buffers = self._records(fields, n, encoder)
                self._check(self.lib.htm_group_run(self._g, banks, chunk + 1, n, 0, int(bool(use_graph)), recs), "htm_group_run")
            finally:
                for e in engines:
                    e.set_run_feedback(None)
                if fields is not None:
                    self._unset_votes()
            for e in engines:
                e.steps += n
            if fields is not None:
                call.add(self._read_records(fields, n, buffers, encoder))
            for i, (e, ptr) in enumerate(zip(engines, ptrs)):
                rows[i, done:done + n] = e.read_bank(ptr, chunk + 1)[(start[i] + np.arange(n)) % (chunk + 1)]
        records = call.finish([steps] * B, [k] * B)
        return rows if fields is None else (rows, records)

    def predicted_value(self, encoder):
        """Every member's predicted_value(encoder): (value float64 [B, F], score int32 [B, F]) -- per member the votes launch, the
        decode launch and a read-back of 2 F ints (htm_predicted_value)."""
        pairs = [m.predicted_value(encoder) for m in self.models]
        return np.stack([v for v, _ in pairs]), np.stack([s for _, s in pairs])

    def forecast_values(self, steps, encoder, min_votes=1, max_bits=0, use_graph=True):
        """Every member's forecast_values(steps, encoder, min_votes, max_bits) at once: (value float64 [B, steps, F], score int32
        [B, steps, F]).  Row 0 of a member is its own predicted_value(); the others come from the group forecast's recorded rows."""
        B, steps = len(self.models), int(steps)
        bucket = np.full((B, max(steps, 0), len(encoder)), -1, dtype=np.int32)
        score = np.zeros_like(bucket)
        if steps > 0:
            for i, m in enumerate(self.models):
                m._forecast_engine("forecast_values()")
                encoder.check_model(m.engine.input_dim, m.engine.column_dim)
                bucket[i, 0], score[i, 0] = m.engine.predicted_value(encoder)
            _, recs = self.forecast(steps, min_votes, max_bits, record=("predicted_value",), use_graph=use_graph, encoder=encoder)
            for i, rec in enumerate(recs):
                bucket[i, 1:], score[i, 1:] = rec.predicted_bucket[:-1], rec.predicted_score[:-1]
        return encoder.value_of(bucket), score

    def process(self, X, learning=None, record=True):
        """One timestep of every member, member i on X[i] (bool [B, input_dim]) -- its own process(X[i]) at once.  Returns a
        RunRecord whose row i is member i's step (its step_index, counters and anomaly_score), or None with record=False.
        learning=None: True, or False in a group with inference views (which refuses True)."""
        learning = self._learning(learning)
        X = np.asarray(X, dtype=np.bool_)
        B = len(self.models)
        e0 = self.models[0].engine
        if X.shape != (B, e0.input_dim):
            raise ValueError(f"X: bool [{B}, {e0.input_dim}], got {X.shape}")
        for m in self.models:
            retire_states(m.engine)
        self._current()
        if self._auto_grow:
            self._grow(self.models[0].active_columns, False)
        words = (e0.input_dim + 31) // 32
        packed = np.ascontiguousarray(np.stack([pack_bits(x, words) for x in X]), dtype=np.uint32)
        steps = [m.engine.steps for m in self.models]
        recs = None
        if record:
            recs, buffers = self._records(("counters",), 1)
        self._check(self.lib.htm_group_step(self._g, packed.ctypes.data_as(C.c_void_p), int(bool(learning)), recs), "htm_group_step")
        for m in self.models:
            m.engine.steps += 1
            m.temporal_memory._new_state(None)
        counters = np.concatenate([r["counters"] for r in self._read_records(("counters",), 1, buffers)]) if record else None
        for m in self.models:                       # (an overflow is reported in the tick it happened, recorded or not)
            m.engine.check_capacity()
        return RunRecord(np.asarray(steps, dtype=np.int64), counters=counters) if record else None

    # ---- live ticks (htm_live_tick / htm_live_reset, include/bithtm_hip.h)
    def _member_mask(self, mask, what):
        """bool [B] (None: `None`), ValueError for another shape."""
        if mask is None:
            return None
        mask = np.asarray(mask)
        if mask.shape != (len(self.models),):
            raise ValueError(f"{what}: bool [{len(self.models)}], got shape {mask.shape}")
        return mask.astype(np.bool_)

    def _due_resets(self, mask):
        """uint8 [B]: the members a device-side reset is due for -- flagged (mask None: all) and past step 0; a fresh member is in
        the empty state already, as TemporalMemory.reset has it."""
        return np.array([(mask is None or bool(mask[i])) and m.engine.steps > 0 for i, m in enumerate(self.models)], dtype=np.uint8)

    def reset(self, members=None):
        """A sequence reset (model.reset()) of the members flagged in `members` (bool [B]; None: all of them), in one launch."""
        mask = self._member_mask(members, "members")
        for m in self.models:
            retire_states(m.engine)
        self._current()
        due = self._due_resets(mask)
        if due.any():
            self._check(self.lib.htm_live_reset(self._g, due.ctypes.data_as(C.c_void_p)), "htm_live_reset")
        for i, m in enumerate(self.models):         # (the host side as the member's own reset() leaves it)
            if mask is None or mask[i]:
                m.temporal_memory._last_ref = None
                m.temporal_memory._was_reset = True

    def tick(self, values, encoder=None, resets=None, learning=None, predicted_input=False, use_graph=True, likelihood=None, classifier=None,
             targets=None, classifier_learning=None, class_distribution=False, knn=None, labels=None, knn_learning=None, knn_votes_all=False):
        """One live timestep of every member in one call whose copies, launches and waits do not depend on B: member i steps on
        values[i] -- float64 [B, F] with `encoder` (a ScalarEncoder; NaN: missing), encoded on the device, else bool
        [B, input_dim] as process() takes it -- after a sequence reset where resets[i] (bool [B], or None).  Returns a GroupTick:
        every member's counters, step index and capacity flags, with an encoder the decoded prediction of its next values, with
        predicted_input=True the votes.  Member i ends as after `if resets[i]: m.reset()` and `m.run(values[i][None], 1,
        learning=learning, encoder=encoder, record=...)`.  A capacity overflow raises CapacityError in the tick where it
        happened; the exception's `.tick` is the finished GroupTick (the other members' results stand).
        learning=None: True, or False in a group with inference views (which refuses True).
        `likelihood`: an AnomalyLikelihood of B streams -- the tick's records are the streams' next step (htm_likelihood_tick: one
        launch more, B doubles more in the copy out) and GroupTick.anomaly_likelihood holds the B values.
        `classifier`: an SDRClassifierBank of B streams (a one-stream SDRClassifier is refused) -- the tick's patterns are the
        streams' next step (htm_classifiers_tick: three launches more when the bank learns, two when it is frozen, whatever B is;
        still one copy in, one copy out and one wait).  `targets`: int [B], each member's bucket of this tick (-1: missing); None
        with `encoder` and a bank made with field=: the bucket of this tick's value (NaN: missing).  `classifier_learning`: None
        follows `learning`.  A member's reset flag also empties its stream's history.  GroupTick.classified_bucket, _probability,
        _value hold the predictions, with class_distribution=True GroupTick.class_distribution all probabilities.
        `knn`: a KNNClassifierBank of B streams (a one-stream KNNClassifier is refused; over views: KNNClassifierBank.shared) -- the
        tick's patterns are the streams' next step (htm_knns_tick: the capture launch, then three launches when any stream stores, two when none does,
        whatever B is; still one copy in, one copy out and one wait; with `classifier` the patterns are captured once).  `labels`:
        int [B], each member's label of this tick (-1, or anything outside [0, knn.labels): none); None: nothing is labelled.
        `knn_learning`: None follows `learning`.  ValueError before anything is enqueued when a labelled stream is full.  A member's
        reset flag does not touch its store.  GroupTick.knn_label, knn_votes, knn_overlap, knn_nearest_slot, knn_nearest_step hold
        the results, with knn_votes_all=True GroupTick.knn_votes_all every label's votes."""
        near = knn if isinstance(knn, KNNClassifierBank) else None
        if near is None:
            _no_knn(knn, "ModelGroup.tick()")
        bank = classifier if isinstance(classifier, SDRClassifierBank) else None
        if bank is None:
            _no_classifier(classifier, "ModelGroup.tick()")
        learning = self._learning(learning)
        B = len(self.models)
        e0 = self.models[0].engine
        cls_learn = False
        if bank is not None:
            if bank.streams != B:
                raise ValueError(f"tick(classifier=): an SDRClassifierBank of {B} streams, got {bank.streams}")
            cls_learn = bool(learning if classifier_learning is None else classifier_learning)
            bank._no_shared_learning(cls_learn)
        elif targets is not None or classifier_learning is not None or class_distribution:
            raise ValueError("tick(): targets=, classifier_learning= and class_distribution= go with classifier=")
        knn_learn = False
        if near is not None:
            if near.streams != B:
                raise ValueError(f"tick(knn=): a KNNClassifierBank of {B} streams, got {near.streams}")
            knn_learn = bool(learning if knn_learning is None else knn_learning)
            near._no_shared_learning(knn_learn)
        elif labels is not None or knn_learning is not None or knn_votes_all:
            raise ValueError("tick(): labels=, knn_learning= and knn_votes_all= go with knn=")
        if likelihood is not None and likelihood.streams != B:
            raise ValueError(f"tick(likelihood=): an AnomalyLikelihood of {B} streams, got {likelihood.streams}")
        _check_encoder(encoder, None, e0.input_dim, e0.column_dim)
        if encoder is None:
            X = np.asarray(values, dtype=np.bool_)
            if X.shape != (B, e0.input_dim):
                raise ValueError(f"values: bool [{B}, {e0.input_dim}], got {X.shape}")
        else:
            X = np.ascontiguousarray(values, dtype=np.float64)
            if X.shape != (B, len(encoder)):
                raise ValueError(f"values: float64 [{B}, {len(encoder)}], got {X.shape}")
        mask = self._member_mask(resets, "resets")
        host_targets = None
        if bank is not None:
            bank._set_shape(*model_shape(e0))
            host_targets = np.ascontiguousarray(self._bank_targets(bank, None if targets is None else np.asarray(targets)[:, None]
                                                                   if np.ndim(targets) == 1 else targets, X[:, None], encoder, "tick")[:, 0])
        host_labels = None
        if near is not None:
            near._set_shape(*model_shape(e0))
            host_labels = near.check_labels(np.full((B, 1), -1) if labels is None else np.asarray(labels)[:, None] if np.ndim(labels) == 1 else labels)
            if host_labels.shape != (B, 1):
                raise ValueError(f"labels: int [{B}], one label per member, got {list(np.shape(labels))}")
            host_labels = np.ascontiguousarray(host_labels[:, 0])
            stored = ((host_labels >= 0) & knn_learn).astype(np.int64)
            near.check_room(stored)
        for m in self.models:
            retire_states(m.engine)
        self._current()
        if self._auto_grow:
            self._grow(self.models[0].active_columns, False)
        flags = self._due_resets(mask) if mask is not None and mask.any() else None
        e0 = self.models[0].engine
        if bank is not None:
            bank._bind(e0)
            if mask is not None:                    # (a flagged member that has not stepped yet gets no device-side reset: its stream's history still goes)
                fresh = np.array([bool(mask[i]) and m.engine.steps == 0 for i, m in enumerate(self.models)])
                if fresh.any():
                    bank.reset(fresh)
        rows = np.zeros(B, dtype=L.HtmLiveRow)
        pairs = votes = None
        if encoder is None:
            words = (e0.input_dim + 31) // 32
            packed = np.ascontiguousarray(np.stack([pack_bits(x, words) for x in X]), dtype=np.uint32)
            args = (None, None, 0, packed.ctypes.data_as(C.c_void_p))
        else:
            pairs = np.zeros((B, len(encoder), 2), dtype=np.int32)
            args = (X.ctypes.data_as(C.c_void_p), encoder.table(), len(encoder), None)
        if predicted_input:
            votes = np.zeros((B, e0.input_dim), dtype=np.int32)

        def ptr(a):
            return None if a is None else a.ctypes.data_as(C.c_void_p)
        scores = best = dist = knn_rows = knn_votes = None
        if bank is not None:
            H = len(bank.steps)
            best = np.zeros((B, H, 2), dtype=np.int32)
            dist = np.zeros((B, H, bank.buckets), dtype=np.int32) if class_distribution else None
        if near is not None:
            near._bind(e0)
            knn_rows = np.zeros((B, 5), dtype=np.int32)
            knn_votes = np.zeros((B, near.labels), dtype=np.int32) if knn_votes_all else None
            lk = None
            if likelihood is not None:
                likelihood._bind(e0)
                scores, lk = np.zeros(B, dtype=np.float64), likelihood._lk
            self._check(self.lib.htm_knns_tick(self._g, *args, ptr(flags), int(bool(learning)), int(bool(use_graph)), ptr(rows), ptr(pairs), ptr(votes), lk,
                                               ptr(scores), bank._clf if bank is not None else None, ptr(host_targets), int(cls_learn), ptr(best), ptr(dist),
                                               near._knn, ptr(host_labels), int(knn_learn), ptr(knn_rows), ptr(knn_votes)), "htm_knns_tick")
            near._counts += stored
            near._total += 1
        elif bank is not None:
            lk = None
            if likelihood is not None:
                likelihood._bind(e0)
                scores, lk = np.zeros(B, dtype=np.float64), likelihood._lk
            self._check(self.lib.htm_classifiers_tick(self._g, *args, ptr(flags), int(bool(learning)), int(bool(use_graph)), ptr(rows), ptr(pairs),
                                                      ptr(votes), lk, ptr(scores), bank._clf, ptr(host_targets), int(cls_learn), ptr(best), ptr(dist)),
                        "htm_classifiers_tick")
        elif likelihood is None:
            self._check(self.lib.htm_live_tick(self._g, *args, ptr(flags), int(bool(learning)), int(bool(use_graph)), ptr(rows), ptr(pairs),
                                               ptr(votes)), "htm_live_tick")
        else:
            likelihood._bind(e0)
            scores = np.zeros(B, dtype=np.float64)
            self._check(self.lib.htm_likelihood_tick(self._g, *args, ptr(flags), int(bool(learning)), int(bool(use_graph)), ptr(rows), ptr(pairs),
                                                     ptr(votes), likelihood._lk, ptr(scores)), "htm_likelihood_tick")
        for m in self.models:
            m.engine.steps += 1
            m.temporal_memory._new_state(None)
        tick = GroupTick(rows, pairs, votes, encoder, scores, best, dist, bank.field if bank is not None else None, knn_rows, knn_votes)
        if tick.capacity_error.any():
            what = "; ".join(f"member {i}:" + "".join(" " + text for bit, text in _CAPACITY_FLAGS if flag & bit) + f" (flags {flag})"
                             for i, flag in enumerate(tick.capacity_error.tolist()) if flag)
            err = CapacityError("capacity exhausted: " + what)
            err.tick = tick
            raise err
        return tick
