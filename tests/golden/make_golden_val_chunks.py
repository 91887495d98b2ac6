#!/usr/bin/env python3
"""Golden vectors of the validation chunker, made by the REFERENCE function itself
(attention_points/scannet_dataset/data_transformation.py:270-331, get_all_subsets_for_scene_numpy,
numpy only).

The function is numpy-only, but its module imports TensorFlow at the top; a MagicMock stands in
for it in sys.modules. Its leftover print("mask", ...) per column is silenced. The scenes are
tests/feed_cases.py's (deterministic numpy PCG64), so the fixture stores, per case, the generator
spec, the np.random seed set before the call, shape, dtype and SHA-256 of every output, and the
first rows of every output for diagnosis (make_golden_scene.py's format).
Run: python tests/golden/make_golden_val_chunks.py <root of the reference checkout>
"""
import contextlib
import importlib
import io
import json
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(reference_root):
    import feed_cases as fc
    sys.path.insert(0, reference_root)
    sys.modules["tensorflow"] = mock.MagicMock()
    dt = importlib.import_module("attention_points.scannet_dataset.data_transformation")
    out = []
    for name, sid, n, npoints, seed in fc.GOLDEN_CASES:
        pts, lab, col, nrm = fc.golden_scene(name, sid, n)
        np.random.seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            res = dt.get_all_subsets_for_scene_numpy(pts, lab, col, nrm, npoints)
        out.append({"name": name, "scene_id": sid, "n_points": n, "npoints": npoints, "seed": seed,
                    "scene_rows": int(len(pts)),
                    "outputs": {k: fc.digest(v) for k, v in zip(fc.OUTPUT_NAMES, res)},
                    "head": {k: np.asarray(v)[0, :4].tolist()
                             for k, v in zip(fc.OUTPUT_NAMES, res)}})
        print(name, sid, n, npoints, seed, {k: np.asarray(v).shape
                                            for k, v in zip(fc.OUTPUT_NAMES, res)})
    with open(os.path.join(HERE, "val_chunks.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
