"""Write tests/golden/metrics_cases.npz: (prediction, y) cases and the tuples the reference's own
tools/evaluate.py returns for them, for tests/test_metrics.py and tests/test_gpu_metrics.py to check
bigcn_amd.metrics against.  CPU only; the test suite only reads the file.

    python tools/gen_metrics_golden.py /path/to/the/reference

The reference's ``evaluation4class`` / ``evaluationclass`` are loaded from ``<reference>/tools/evaluate.py``
and CALLED (on plain Python int lists); nothing of their text is kept.  The file holds arrays only:

* ``names4`` / ``names2``: the cases' names; per case ``<name>:pred``, ``<name>:y`` (int64) and
  ``<name>:ref`` (float64, the 17 / 9 numbers returned);
* one "epoch" of three ragged 4-class batches ``epoch:pred:<k>``, ``epoch:y:<k>``, made-up fp32 losses
  ``epoch:loss``, ``epoch:tuples`` [3, 17] (the reference's tuple per batch) and what its test loop
  (BiGCN_Twitter.py:219-247) makes of them, restated here as that loop has it - ``np.mean`` of the
  appended ``.item()`` values: ``epoch:loss_mean``, ``epoch:acc_mean``, ``epoch:mean`` [17];
* ``epoch:conf`` [4, 4] and ``epoch:precision`` / ``epoch:recall`` / ``epoch:f1`` [4]: the explain run's
  float confusion matrix over the same trees and its unrounded per-class numbers, restated as
  explain_PHEME.py:480, 609, 652-659 has them (class 3 is never a label there: 0 / 0 = nan).
"""
import argparse
import importlib.util
import os
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_reference(ref_dir):
    path = os.path.join(ref_dir, "tools", "evaluate.py")
    spec = importlib.util.spec_from_file_location("reference_evaluate", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases4(rng):
    def rand(n, hi_y=4, hi_p=4):
        return rng.integers(0, hi_p, size=n).tolist(), rng.integers(0, hi_y, size=n).tolist()

    yield "b1_right", ([2], [2])
    yield "b1_wrong", ([1], [3])
    yield "one_class", ([1] * 9, [1] * 9)
    yield "never_predicted", ([0, 1, 3, 3, 0, 1, 1], [0, 1, 2, 3, 2, 1, 0])       # nothing predicted as 2
    yield "never_present", ([0, 1, 3, 2, 0, 1, 2, 3, 1], [0, 1, 2, 2, 0, 1, 1, 0, 2])   # no label 3
    yield "prec_recll_zero", ([1, 1, 0, 2, 2], [0, 0, 1, 2, 3])     # classes 0, 1: TP = 0 with FP, FN > 0
    for n in (3, 7, 9, 11):
        yield f"rand{n}", rand(n)
    yield "label_ge4", ([0, 1, 5, 3, 2, 1, 4, 0, 3, 15, 2], [0, 4, 2, 3, 7, 1, 4, 0, 2, 15, 1])
    yield "rand128", rand(128)
    yield "rand257_skewed", (rng.choice(4, size=257, p=[0.7, 0.2, 0.1, 0.0]).tolist(),
                             rng.choice(4, size=257, p=[0.6, 0.1, 0.0, 0.3]).tolist())


def cases2(rng):
    yield "b1", ([0], [0])
    yield "b1_wrong", ([0], [1])
    yield "all_zero", ([0] * 7, [0] * 7)
    yield "never_predicted", ([0, 0, 0], [0, 1, 1])
    yield "prec_recll_zero", ([1, 0, 1], [0, 1, 0])
    for n in (3, 7, 9, 11, 128):
        yield f"rand{n}", (rng.integers(0, 2, size=n).tolist(), rng.integers(0, 2, size=n).tolist())
    yield "label_ge2", ([0, 1, 2, 1, 0, 3, 1], [0, 1, 1, 2, 0, 3, 0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="the reference's directory (holds tools/evaluate.py)")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    rng = np.random.default_rng(31)
    out = {}
    for key, gen, fn in (("names4", cases4, ref.evaluation4class), ("names2", cases2, ref.evaluationclass)):
        names = []
        for name, (pred, y) in gen(rng):
            name = f"{key[-1]}:{name}"
            names.append(name)
            out[name + ":pred"] = np.array(pred, dtype=np.int64)
            out[name + ":y"] = np.array(y, dtype=np.int64)
            out[name + ":ref"] = np.array(fn(pred, y), dtype=np.float64)
        out[key] = np.array(names)
    # one epoch: three ragged batches; labels 0..2 only, class 3 sometimes predicted
    batches = [(rng.integers(0, 4, size=n).tolist(), rng.integers(0, 3, size=n).tolist()) for n in (7, 5, 3)]
    losses = np.array([1.3862944, 0.9713216, 1.1020054], dtype=np.float32)
    tuples, temp_losses, temp_accs = [], [], []
    conf = np.zeros((4, 4))
    for k, (pred, y) in enumerate(batches):
        out[f"epoch:pred:{k}"] = np.array(pred, dtype=np.int64)
        out[f"epoch:y:{k}"] = np.array(y, dtype=np.int64)
        temp_losses.append(losses[k].item())
        correct = int((np.array(pred) == np.array(y)).sum())
        temp_accs.append(correct / len(y))
        tuples.append(ref.evaluation4class(pred, y))
        for p, a in zip(pred, y):
            conf[a, p] += 1
    out["epoch:loss"] = losses
    out["epoch:tuples"] = np.array(tuples, dtype=np.float64)
    out["epoch:loss_mean"] = np.float64(np.mean(temp_losses))
    out["epoch:acc_mean"] = np.float64(np.mean(temp_accs))
    out["epoch:mean"] = np.array([np.mean([t[j] for t in tuples]) for j in range(17)], dtype=np.float64)
    prec, rec, f1 = np.zeros(4), np.zeros(4), np.zeros(4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(4):
            prec[i] = conf[i, i] / conf[:, i].sum()
            rec[i] = conf[i, i] / conf[i, :].sum()
            f1[i] = 2 * prec[i] * rec[i] / (prec[i] + rec[i])
    out.update({"epoch:conf": conf.astype(np.int64), "epoch:precision": prec, "epoch:recall": rec, "epoch:f1": f1})
    path = os.path.join(ROOT, "tests", "golden", "metrics_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{len(out['names4'])} four-class and {len(out['names2'])} two-class cases, one epoch of "
          f"{len(batches)} batches: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
