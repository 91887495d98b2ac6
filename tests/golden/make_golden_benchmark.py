#!/usr/bin/env python3
"""Golden vectors of the ScanNet benchmark score, made by the REFERENCE module itself
(attention_points/benchmark/evaluate.py, numpy only).

Three small synthetic scenes of predicted / ground-truth NYU-40 ids (numpy RandomState, stored in
the fixture as they are): they hold ground-truth ids outside VALID_CLASS_IDS (skipped),
predictions outside it (counted as UNKNOWN_ID), and class 36 (bathtub) occurs in neither list of
the first two scenes, so its IoU is NaN until the third scene adds it. After each scene the
fixture records the reference's cumulative 41 x 41 confusion matrix and get_iou of every valid id
([iou, tp, denom], or null for NaN; the float as repr() for an exact comparison), and at the end
the text of write_result_file.

Run: python tests/golden/make_golden_benchmark.py <root of the reference checkout>
"""
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

VALID = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
INVALID_GT = [0, 13, 15, 40, 41, 255, -1]
INVALID_PRED = [0, 13, 17, 40, 100, -3]
SCENES = [  # (seed, points, classes left out)
    (1, 400, (36,)),
    (2, 257, (36, 28)),
    (3, 600, ()),
]


def make_scene(seed, n, without):
    rng = np.random.RandomState(seed)
    classes = [c for c in VALID if c not in without]
    gt = rng.choice(classes, n)
    # two thirds of the predictions are right, the others are some valid class
    pred = np.where(rng.uniform(size=n) < 0.66, gt, rng.choice(classes, n))
    bad_gt, bad_pred = rng.uniform(size=n) < 0.1, rng.uniform(size=n) < 0.08
    gt = np.where(bad_gt, rng.choice(INVALID_GT, n), gt)
    pred = np.where(bad_pred, rng.choice(INVALID_PRED, n), pred)
    return [int(v) for v in pred], [int(v) for v in gt]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    spec = importlib.util.spec_from_file_location(
        "reference_evaluate", os.path.join(sys.argv[1], "attention_points", "benchmark", "evaluate.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    assert [int(v) for v in ref.VALID_CLASS_IDS] == VALID
    n = int(ref.UNKNOWN_ID) + 1
    confusion = np.zeros((n, n), dtype=np.ulonglong)
    scenes = []
    with tempfile.TemporaryDirectory() as tmp:
        for seed, npts, without in SCENES:
            pred, gt = make_scene(seed, npts, without)
            files = []
            for name, ids in (("pred", pred), ("gt", gt)):
                files.append(os.path.join(tmp, f"{name}{seed}.txt"))
                with open(files[-1], "w") as f:
                    f.write("".join("%d\n" % v for v in ids))
            ref.evaluate_scan(files[0], files[1], confusion)
            ious = []
            for label_id in VALID:
                v = ref.get_iou(label_id, confusion)
                ious.append(None if isinstance(v, float) else [repr(float(v[0])), int(v[1]), int(v[2])])
            scenes.append({"pred": pred, "gt": gt, "confusion": confusion.astype(np.int64).tolist(),
                           "ious": ious})
            print(seed, npts, int(confusion.sum()), sum(v is None for v in ious), "NaN")
        class_ious = {ref.CLASS_LABELS[i]: ref.get_iou(VALID[i], confusion) for i in range(len(VALID))}
        path = os.path.join(tmp, "result.txt")
        ref.write_result_file(confusion, class_ious, path)
        text = open(path).read()
    out = {"valid_class_ids": VALID, "class_labels": list(ref.CLASS_LABELS),
           "unknown_id": int(ref.UNKNOWN_ID), "scenes": scenes, "result_file": text}
    with open(os.path.join(HERE, "benchmark_eval.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))


if __name__ == "__main__":
    main()
