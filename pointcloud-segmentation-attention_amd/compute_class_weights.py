"""attention_points/scannet_dataset/compute_class_weights.py: the class weights of the training
loss from the label distribution of the training scenes.

    weights_from_counts(counts)   1 / log(1.2 + counts / sum(counts)) in float64 (:34-36, the
                                  formula adapted from Charles Qi's implementation)
    get_weights(label_arrays)     the counts of the mapped labels of every scene, then the formula

Class 0 is unannotated and is weighted 0 by the training loop (train.CLASS_WEIGHTS[0]); the
formula's own value for it is returned here as the reference returns it.
"""
import numpy as np
import torch

from .data_transformation import _label_lut

NUM_CLASSES = 21


def weights_from_counts(counts):
    """1 / log(1.2 + counts / sum(counts)), float64 (:35-36)."""
    counts = np.asarray(counts)
    return 1 / np.log(1.2 + counts / np.sum(counts))


def get_weights(label_arrays):
    """:13-37 over an iterable of per-scene label arrays (NYU-40 ids, numpy or tensors): each
    scene's labels are mapped to 0..20 (LABEL_MAP.get(label, 0), torch.ops.pn2.label_lut) and
    counted on the labels' device; the 21 int64 counts are read back once, after the last scene.
    Returns (weights (21,) float64, counts (21,) int64)."""
    total = None
    for labels in label_arrays:
        t = labels if isinstance(labels, torch.Tensor) else \
            torch.from_numpy(np.ascontiguousarray(np.asarray(labels)))
        mapped = _label_lut(t.clamp(-1, 2 ** 31 - 1).to(torch.int32).reshape(-1).contiguous())
        cnt = torch.bincount(mapped.to(torch.int64), minlength=NUM_CLASSES)
        total = cnt if total is None else total.to(cnt.device) + cnt
    if total is None:
        total = torch.zeros(NUM_CLASSES, dtype=torch.int64)
    counts = total.cpu().numpy()
    return weights_from_counts(counts), counts
