"""attention_points/benchmark/generate_predictions.py: a label for every point of a scene.

The reference runs the model on every chunk of the whole-scene chunker, takes np.argmax of the
logits on the host, concatenates a scene's chunks and calls map_back (:19-37) three times
(predictions, points, labels), then map_to_nyu40 (:40-53) and export_ids (:56-65). Here the
argmax and map_back are the kernels of csrc/predict.hip (torch.ops.pn2.scene_vote, scene_labels,
map_back_rows, label_lut): every scene point holds the 64-bit key ((global row + 1) << 8) | label
and every masked row applies an integer atomic max to its point's key. The largest row wins,
which is numpy's order for repeated indices (a point on a column boundary lies in two inner
boxes), and the max commutes, so a scene streams through the model batch by batch and its logits
never reach the host.

    map_back, map_to_nyu40, export_ids   the reference's functions
    predict_scene                        one scene: chunk, model, vote per batch, resolve once
    generate_predictions                 scenes -> the reference's output files

The four ops also have CPU kernels (host twins, equal bits), which is what map_back and
map_to_nyu40 run for numpy inputs.
"""
import os

import numpy as np
import torch

from . import _torch_ops, complete_scene_loader

N_POINTS = 8192  # :11
# :48-50, the ScanNet labels 1..20 as NYU-40 ids; dict.get(label, 1): 0 and anything unknown -> 1
NYU40_LABELS = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10, 11: 11, 12: 12,
                13: 14, 14: 16, 15: 24, 16: 28, 17: 33, 18: 34, 19: 36, 20: 39}
NYU40_LUT = [NYU40_LABELS.get(i, 1) for i in range(21)]
NYU40_DEFAULT = 1


def _lut(table, device):
    return torch.tensor(table, dtype=torch.int32, device=device)


def _vote_keys(original_idx, mask, n_scene):
    """The keys of rows that carry no logits: only the winning row matters."""
    keys = torch.zeros(n_scene, dtype=torch.int64, device=mask.device)
    _torch_ops.call("scene_vote", None, mask, original_idx, 0, keys)
    return keys


def map_back(values, original_idx, mask, res_shape):
    """:19-37: res = zeros(res_shape); res[original_idx[mask]] = values[mask], the later row
    winning where an index repeats.

    numpy inputs give the reference's result: a float64 array of res_shape (computed by the host
    twins); a masked index >= res_shape[0] raises IndexError and a negative one counts from the
    end, as numpy does. Device (or CPU) tensors give a tensor of the values' dtype on their
    device, whose rows must be a multiple of 4 bytes; there a masked index outside
    [0, res_shape[0]) is ignored."""
    if isinstance(values, torch.Tensor):
        shape = (res_shape,) if isinstance(res_shape, int) else tuple(res_shape)
        n = int(shape[0])
        mask = torch.as_tensor(mask).reshape(-1).to(values.device)
        mask = mask if mask.dtype in (torch.bool, torch.uint8) else mask != 0
        original_idx = torch.as_tensor(original_idx).reshape(-1).to(values.device, torch.int32)
        values = values.reshape((mask.numel(),) + shape[1:])
        keys = _vote_keys(original_idx, mask, n)
        out = torch.empty(shape, dtype=values.dtype, device=values.device)
        _torch_ops.call("map_back_rows", values, 0, keys, out)
        return out
    res = np.zeros(res_shape)
    n = res.shape[0]
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    idx = np.asarray(original_idx).reshape(-1).astype(np.int64)
    hit = idx[mask]
    if hit.size and (hit.max() >= n or hit.min() < -n):
        bad = hit[(hit >= n) | (hit < -n)][0]
        raise IndexError(f"index {bad} is out of bounds for axis 0 with size {n}")
    idx = np.where(idx < 0, idx + n, idx)
    idx = np.where((idx >= 0) & (idx < n), idx, -1).astype(np.int32)  # unmasked rows: never read
    vals = np.ascontiguousarray(np.asarray(values), dtype=np.float64).reshape((mask.size,) +
                                                                              res.shape[1:])
    keys = _vote_keys(torch.from_numpy(idx), torch.from_numpy(mask), n)
    out = torch.from_numpy(res)
    _torch_ops.call("map_back_rows", torch.from_numpy(vals), 0, keys, out)
    return res


def map_to_nyu40(labels):
    """:40-53: the ScanNet labels 1..20 as NYU-40 ids; 0 and every other value give 1
    (dict.get(label, 1)). A numpy array or list gives an array of np.array(labels)'s dtype, as
    the reference (its values are integers, stored as float64 after map_back); a tensor gives an
    int32 tensor on its device."""
    if isinstance(labels, torch.Tensor):
        return _torch_ops.call("label_lut", labels.to(torch.int32), _lut(NYU40_LUT, labels.device),
                               NYU40_DEFAULT)
    labels = np.array(labels)
    # not a whole number, or outside int32: no key of the dict, so -1 -> the default
    f = labels.astype(np.float64)
    with np.errstate(invalid="ignore"):
        known = np.isfinite(f) & (f == np.floor(f)) & (np.abs(f) < 2 ** 31)
    as_int = np.where(known, f, -1.0).astype(np.int32)
    out = _torch_ops.call("label_lut", torch.from_numpy(np.ascontiguousarray(as_int)),
                          _lut(NYU40_LUT, "cpu"), NYU40_DEFAULT)
    return out.numpy().astype(labels.dtype)


def export_ids(filename, ids):
    """:56-65: one id per line."""
    with open(filename, "w") as f:
        for id in ids:
            f.write("%d\n" % id)


def predict_scene(model, points, colors=None, normals=None, labels=None, batch=16,
                  device="cuda"):
    """Labels for every point of one scene, generate_predictions.py:139-186 without the files.

    points (N, 3) float32, colors (N, 3) in 0..255, normals (N, 3), labels (N,) or None, numpy
    arrays. The scene is cut by complete_scene_loader (the `_numpy` variant when labels are
    given, the `_test` variant otherwise: their shuffles come from numpy's global RandomState, so
    np.random.seed fixes the result). `model(xyz (b, 8192, 3), feats (b, 8192, 6) or None)`
    returns logits (b, 8192, C) on the device; it is called on batches of up to `batch` chunks,
    the last one may be smaller; feats = [colors / 255, normals] (:87-88) when colours and
    normals are given, else None. Each batch votes as soon as its logits exist
    (torch.ops.pn2.scene_vote) and the keys are resolved once.

    Returns device tensors: 'labels' (N,) int32, the remapped prediction, 0 where no masked row
    names the point; 'nyu40' (N,) int32 = map_to_nyu40(labels); 'points' (N, 3) float32, the
    winning rows' coordinates (zeros where unwritten); 'gt_labels' (N,) int32 when labels were
    given; 'winner' (N,) int64, the global chunk row that wrote each point, -1 for none."""
    dev = torch.device(device)
    pts = np.ascontiguousarray(points, dtype=np.float32)
    N = int(pts.shape[0])
    with_feats = colors is not None and normals is not None
    col = np.zeros((N, 3), np.int32) if colors is None else np.asarray(colors)
    nrm = np.zeros((N, 3), np.float32) if normals is None else np.asarray(normals)
    csl = complete_scene_loader
    if labels is not None:
        point_sets, label_sets, color_sets, normal_sets, _, masks, orig = \
            csl.get_all_subsets_with_all_points_for_scene_numpy(pts, np.asarray(labels), col, nrm)
    else:
        point_sets, color_sets, normal_sets, masks, orig = \
            csl.get_all_subsets_with_all_points_for_scene_numpy_test(pts, col, nrm)
        label_sets = None
    X = int(point_sets.shape[0])
    xyz = torch.from_numpy(np.ascontiguousarray(point_sets, dtype=np.float32)).to(dev)
    feats = None
    if with_feats:  # :87-88
        c = torch.from_numpy(np.ascontiguousarray(color_sets)).to(dev).to(torch.float32) / 255.0
        feats = torch.cat([c, torch.from_numpy(np.ascontiguousarray(normal_sets, dtype=np.float32))
                           .to(dev)], dim=2).contiguous()
    mask = torch.from_numpy(np.ascontiguousarray(masks, dtype=bool)).to(dev)
    orig = torch.from_numpy(np.ascontiguousarray(orig).astype(np.int32)).to(dev)
    keys = torch.zeros(N, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for b0 in range(0, X, int(batch)):
            b1 = min(X, b0 + int(batch))
            logits = model(xyz[b0:b1], None if feats is None else feats[b0:b1])
            _torch_ops.call("scene_vote", logits, mask[b0:b1], orig[b0:b1], b0 * N_POINTS, keys)
    pred, nyu40, winner = _torch_ops.call("scene_labels", keys, _lut(NYU40_LUT, dev),
                                          NYU40_DEFAULT)
    out = {"labels": pred, "nyu40": nyu40, "winner": winner,
           "points": torch.empty((N, 3), dtype=torch.float32, device=dev)}
    _torch_ops.call("map_back_rows", xyz.reshape(-1, 3), 0, keys, out["points"])
    if label_sets is not None:
        gt = torch.from_numpy(np.ascontiguousarray(label_sets).astype(np.int32)).to(dev)
        out["gt_labels"] = torch.empty(N, dtype=torch.int32, device=dev)
        _torch_ops.call("map_back_rows", gt.reshape(-1), 0, keys, out["gt_labels"])
    return out


def generate_predictions(model, scenes, out_dir, batch=16, device="cuda"):
    """:94-186 over an iterable of (name, points, colors, normals, labels or None): writes, in the
    reference's layout and dtypes (map_back's float64 arrays),
        out_dir/points/NAME.npy              (N, 3)
        out_dir/labels/NAME.npy              (N,)  the prediction, ScanNet labels 0..20
        out_dir/groundtruth_labels/NAME.npy  (N,)  when labels were given
        out_dir/predictions/NAME.txt         the NYU-40 ids, one per line (export_ids)
    Returns the scene names."""
    for sub in ("points", "labels", "groundtruth_labels", "predictions"):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
    names = []
    for name, points, colors, normals, labels in scenes:
        res = predict_scene(model, points, colors, normals, labels, batch=batch, device=device)
        host = {k: v.cpu().numpy() for k, v in res.items()}
        np.save(os.path.join(out_dir, "points", f"{name}.npy"), host["points"].astype(np.float64))
        np.save(os.path.join(out_dir, "labels", f"{name}.npy"), host["labels"].astype(np.float64))
        if "gt_labels" in host:
            np.save(os.path.join(out_dir, "groundtruth_labels", f"{name}.npy"),
                    host["gt_labels"].astype(np.float64))
        export_ids(os.path.join(out_dir, "predictions", f"{name}.txt"), host["nyu40"])
        names.append(name)
    return names
