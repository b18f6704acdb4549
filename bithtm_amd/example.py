"""Harness for the MI355X engine with the command line, input model and per-step report of the
reference's example script (flags: example.py:22-30; random pattern bank: :34; flip noise: :52;
the three counters: :55-57), so that its output can be compared line by line.

    python -m bithtm_amd.example --epochs 8
    python -m bithtm_amd.example --epochs 8 --batched   # one C-ABI call per epoch, hipGraph replay
    python -m bithtm_amd.example --epochs 8 --batched_report   # ... recorded: the per-step lines of the default mode
    python -m bithtm_amd.example --epochs 8 --batched_report --likelihood   # ... with each step's anomaly likelihood
    python -m bithtm_amd.example --epochs 8 --batched_report --classifier   # ... with an SDR classifier's 1-step hit rate per epoch
    python -m bithtm_amd.example --epochs 8 --batched_report --knn   # ... a KNN classifier stores the first epochs' labelled steps, names the later ones
    python -m bithtm_amd.example --epochs 8 --batched --device_noise   # ... the bank uploaded once, the flip noise drawn on the device
    python -m bithtm_amd.example --epochs 8 --sequence_length 10   # a sequence reset before every 10th pattern
    python -m bithtm_amd.example --epochs 8 --use_reference_implementation   # example.py:30,36-37 (needs the user's `bithtm`)
"""

import argparse
import sys
import time

import numpy as np

from bithtm_amd import AnomalyLikelihood, HierarchicalTemporalMemory, KNNClassifier, SDRClassifier

FLAGS = (
    # name, type, default  (the reference's flags, same names and defaults)
    ("epochs", int, 100),
    ("input_patterns", int, 100),
    ("input_dim", int, 1000),
    ("input_density", float, 0.2),
    ("input_noise_probability", float, 0.05),
    ("column_dim", int, 2048),
    ("cell_dim", int, 32),
)


def parse(argv):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for name, kind, default in FLAGS:
        ap.add_argument("--" + name, type=kind, default=default)
    ap.add_argument("--use_reference_implementation", action="store_true",
                    help="the reference's flag (example.py:30): swap the Temporal Memory for the textbook one of the user's own "
                         "`bithtm.reference_implementations` (example.py:7-12, 36-37); the Spatial Pooler stays on the device")
    ap.add_argument("--seed", type=int, default=0, help="seed of the Temporal Memory's keyed random draws")
    ap.add_argument("--batched", action="store_true",
                    help="run each epoch with HierarchicalTemporalMemory.run (no per-step read-back) and "
                         "report timesteps/s per epoch instead of the per-step counters")
    ap.add_argument("--batched_report", action="store_true",
                    help="run each epoch as one recorded HierarchicalTemporalMemory.run and print the per-step counters "
                         "from its record (the same lines as the default mode)")
    ap.add_argument("--sequence_length", type=int, default=0,
                    help="the bank is sequences of this many patterns: a sequence reset before every such pattern (0: none).  "
                         "Stepwise with the reference's idiom, `last_state = get_empty_state()`; batched with run(resets=)")
    ap.add_argument("--device_noise", action="store_true",
                    help="with --batched / --batched_report: upload the bank once and draw the flip noise on the device "
                         "(run(noise=): the keyed generator under --seed, a fresh draw per timestep) instead of drawing it with "
                         "np.random and uploading a noisy bank per epoch")
    ap.add_argument("--likelihood", action="store_true",
                    help="with --batched_report: score every step's anomaly likelihood on the device (run(likelihood=), NuPIC's "
                         "default parameters, one stream over all epochs) and print it as a further column")
    ap.add_argument("--classifier", action="store_true",
                    help="with --batched_report: learn an SDR classifier on the device from each step's active cells to the index of the "
                         "pattern one step ahead (run(classifier=), one bucket per pattern) and print its 1-step hit rate per epoch")
    ap.add_argument("--knn", action="store_true",
                    help="with --batched_report: label each step of the first half of the epochs with its pattern's index and store its "
                         "active cells in a KNN classifier on the device (run(knn=), k = 3); print the hit rate of the later epochs")
    return ap.parse_args(argv)


def epoch_input(bank, opts):
    """(rows, run()'s noise arguments) of one batched epoch: the bank itself and the device's noise, or a host-drawn noisy bank."""
    if opts.device_noise:
        return bank, dict(noise=opts.input_noise_probability)
    return bank ^ (np.random.rand(*bank.shape) < opts.input_noise_probability), {}


def reset_rows(opts):
    """The patterns a sequence starts with (a reset before each), or None."""
    if opts.sequence_length <= 0:
        return None
    return np.arange(opts.input_patterns) % opts.sequence_length == 0


def digits(n):
    """Field width the reference uses for a counter that can reach n - 1."""
    return int(np.ceil(np.log10(max(n - 1, 2))))


class Report:
    """Formats one line per timestep exactly like the reference's print statement."""

    def __init__(self, opts, active_columns):
        self.w_epoch, self.w_pattern = digits(opts.epochs), digits(opts.input_patterns)
        self.w_column, self.w_active = digits(opts.column_dim), digits(active_columns)

    def line(self, epoch, pattern, bursting, correct, incorrect):
        return (f"epoch {epoch:{self.w_epoch}d}, pattern {pattern:{self.w_pattern}d}: "
                f"bursting columns: {bursting:{self.w_active}d}, correct columns: {correct:{self.w_active}d}, "
                f"incorrect columns: {incorrect:{self.w_column}d}")


def column_counters(predicted_columns, sp_state, tm_state):
    """(bursting, correctly predicted, incorrectly predicted) columns of one timestep."""
    hit = int(predicted_columns[sp_state.active_column].sum())
    return int(tm_state.active_column_bursting.sum()), hit, int(predicted_columns.sum()) - hit


def run_stepwise(htm, bank, opts, out):
    report = Report(opts, htm.spatial_pooler.active_columns)
    for epoch in range(opts.epochs):
        for index, pattern in enumerate(bank):
            if opts.sequence_length > 0 and index % opts.sequence_length == 0:
                htm.temporal_memory.last_state = htm.temporal_memory.get_empty_state()
            predicted_columns = htm.temporal_memory.last_state.cell_prediction.any(axis=1)
            flips = np.random.rand(opts.input_dim) < opts.input_noise_probability
            states = htm.process(pattern ^ flips)
            print(report.line(epoch, index, *column_counters(predicted_columns, *states)), file=out)


def run_batched(htm, bank, opts, out):
    width = digits(opts.epochs)
    for epoch in range(opts.epochs):
        noisy, noise = epoch_input(bank, opts)
        began = time.time()
        htm.run(noisy, len(noisy), resets=reset_rows(opts), **noise)
        htm.engine.sync()
        rate = len(noisy) / (time.time() - began)
        print(f"epoch {epoch:{width}d}: {rate:.0f} timesteps/s, {htm.engine.info().segments} segments", file=out)


def run_batched_report(htm, bank, opts, out):
    # (one draw of the epoch's noise: the same MT19937 values, in the same order, as run_stepwise's draw per step)
    report = Report(opts, htm.spatial_pooler.active_columns)
    scoring = dict(likelihood=AnomalyLikelihood()) if opts.likelihood else {}
    if opts.classifier:                             # (a step's target is its own pattern's index: horizon 1 learns the one that follows)
        scoring.update(classifier=SDRClassifier(buckets=len(bank), steps=(1,), alpha=0.1), targets=np.arange(len(bank)))
    labelled = max(opts.epochs // 2, 1)             # (--knn: the epochs whose steps are labelled and stored)
    if opts.knn:
        scoring.update(knn=KNNClassifier(len(bank), k=3, capacity=len(bank) * labelled))
    for epoch in range(opts.epochs):
        noisy, noise = epoch_input(bank, opts)
        if opts.knn:
            scoring.update(labels=np.arange(len(bank)) if epoch < labelled else None)
        rec = htm.run(noisy, len(noisy), record=True, resets=reset_rows(opts), **noise, **scoring)
        for index, (b, c, i) in enumerate(zip(rec.bursting_columns, rec.correct_columns, rec.incorrect_columns)):
            scored = f", anomaly likelihood: {rec.anomaly_likelihood[index]:.6f}" if opts.likelihood else ""
            print(report.line(epoch, index, int(b), int(c), int(i)) + scored, file=out)
        if opts.classifier:
            hits = rec.classified_bucket[:, 0] == (np.arange(len(bank)) + 1) % len(bank)
            print(f"epoch {epoch:{report.w_epoch}d}: 1-step hit rate of the classifier: {hits.mean():.3f}", file=out)
        if opts.knn and epoch >= labelled:
            hits = rec.knn_label == np.arange(len(bank))
            print(f"epoch {epoch:{report.w_epoch}d}: hit rate of the KNN classifier over {scoring['knn'].count} stored steps: {hits.mean():.3f}", file=out)


def main(argv=None, out=sys.stdout):
    opts = parse(argv)
    bank = np.random.rand(opts.input_patterns, opts.input_dim) < opts.input_density
    if opts.use_reference_implementation:
        # example.py:7-12: the same network with `temporal_memory=` the textbook implementation -- the user's package, imported
        # at the user's request (this package ships no copy of it and no CPU path of its own)
        if opts.batched or opts.batched_report:
            raise SystemExit("--batched / --batched_report run the fused device step; --use_reference_implementation steps a host-side Temporal Memory")
        try:
            from bithtm.reference_implementations import TemporalMemory as ReferenceTemporalMemory
        except ImportError as e:
            raise SystemExit(f"--use_reference_implementation needs the reference's `bithtm` package on PYTHONPATH ({e})")
        htm = HierarchicalTemporalMemory(opts.input_dim, opts.column_dim, opts.cell_dim,
                                         temporal_memory=ReferenceTemporalMemory(opts.column_dim, opts.cell_dim))
    else:
        if opts.likelihood and not opts.batched_report:
            raise SystemExit("--likelihood prints a column of the recorded report: use it with --batched_report")
        if opts.classifier and not opts.batched_report:
            raise SystemExit("--classifier rides on the recorded report's runs: use it with --batched_report")
        if opts.classifier and opts.input_patterns > 1024:
            raise SystemExit("--classifier: one bucket per pattern, at most 1024 patterns")
        if opts.knn and not opts.batched_report:
            raise SystemExit("--knn rides on the recorded report's runs: use it with --batched_report")
        if opts.knn and opts.input_patterns > 1024:
            raise SystemExit("--knn: one label per pattern, at most 1024 patterns")
        if opts.device_noise and not (opts.batched or opts.batched_report):
            raise SystemExit("--device_noise draws the noise inside a batched run: use it with --batched or --batched_report")
        htm = HierarchicalTemporalMemory(opts.input_dim, opts.column_dim, opts.cell_dim, seed=opts.seed)
    began = time.time()
    (run_batched if opts.batched else run_batched_report if opts.batched_report else run_stepwise)(htm, bank, opts, out)
    print(f"{time.time() - began} seconds.", file=out)


if __name__ == "__main__":
    main()
