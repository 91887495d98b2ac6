"""Shared by tests/test_feed_cpu.py, tests/test_gpu_feed.py and
tests/golden/make_golden_val_chunks.py: the scenes of the validation chunker's golden cases and
the numpy statements the feed kernels are compared with. Not a test module."""
import hashlib
import importlib

import numpy as np

from support import raw_bits as bits  # noqa: F401  (used as fc.bits)

PKG_NAME = "pointcloud-segmentation-attention_amd"

# (name, scene_id, n_points, npoints, np.random seed) of tests/golden/val_chunks.json
GOLDEN_CASES = (("scene1", 1, 20000, 512, 7), ("scene2", 2, 45000, 512, 11),
                ("skip_path", 5, 6000, 256, 3))
OUTPUT_NAMES = ("point_sets", "labels", "colors", "normals", "sample_weights")


def digest(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": str(a.dtype),
            "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def column_box(pts, i, j, grow):
    """x/y bounds of column (i, j) of the chunker's 1.5 m grid, grown by `grow` on every side."""
    lo = pts.min(axis=0)[:2].astype(np.float64) + [i * 1.5, j * 1.5]
    return lo - grow, lo + 1.5 + grow


def remove_columns(scene, holes):
    """The scene without the points inside the grown columns `holes` = ((i, j, grow), ...); the
    four points at the x / y extremes stay, so the bounding box and the grid do not move."""
    pts = scene[0]
    keep = np.ones(len(pts), bool)
    for i, j, grow in holes:
        lo, hi = column_box(pts, i, j, grow)
        xy = pts[:, :2].astype(np.float64)
        keep &= ~np.all((xy >= lo) & (xy <= hi), axis=1)
    for ax in (0, 1):
        keep[np.argmin(pts[:, ax])] = True
        keep[np.argmax(pts[:, ax])] = True
    return tuple(a[keep] for a in scene)


def skip_path_scene(n_points=6000):
    """synth.scannet_scene(5, n) with column (1,1) grown by 0.002 m emptied (its 0.2 m margin
    still selects points, none of them inside: drawn for, then skipped) and column (3,0) grown
    by 0.25 m emptied (it and the sliver column (4,0) select nothing: no draw)."""
    synth = importlib.import_module(PKG_NAME).synth
    return remove_columns(synth.scannet_scene(5, n_points), ((1, 1, 0.002), (3, 0, 0.25)))


def golden_scene(name, scene_id, n_points):
    if name == "skip_path":
        return skip_path_scene(n_points)
    return importlib.import_module(PKG_NAME).synth.scannet_scene(scene_id, n_points)


def feed_batch_numpy(points, labels, colors, normals, sample_weight, cs, class_weights,
                     use_color, use_normal):
    """The statement pn2_feed_batch is pinned to, in float32 ufuncs (one rounding each; numpy's
    matmul may fuse and is not the yardstick)."""
    f32 = np.float32
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    if cs is None:
        xyz = points.copy()
    else:
        c, s = cs[:, 0:1].astype(f32), cs[:, 1:2].astype(f32)
        xyz = np.stack([x * c + y * s, y * c - x * s, z], axis=-1).astype(f32)
    feats = []
    if use_color:
        feats.append(colors.astype(f32) / f32(255.0))
    if use_normal:
        if cs is None:
            feats.append(normals)
        else:
            nx, ny, nz = normals[..., 0], normals[..., 1], normals[..., 2]
            feats.append(np.stack([nx * c + ny * s, ny * c - nx * s, nz], axis=-1).astype(f32))
    B, N = labels.shape
    features = np.concatenate(feats, axis=-1) if feats else np.zeros((B, N, 0), f32)
    L = len(class_weights)
    ok = (labels >= 0) & (labels < L)
    w = np.where(ok, np.asarray(class_weights, f32)[np.clip(labels, 0, max(L - 1, 0))], f32(0)) \
        if L else np.zeros(labels.shape, f32)
    mask = (sample_weight != 0).astype(f32)
    return xyz, features.astype(f32), (w.astype(f32) * mask).astype(f32)
