"""The crop sampler of attention_points/scannet_dataset/data_transformation.py on gfx950.

get_subset (:70-154) picks a random 1.5 m x 1.5 m column of a ScanNet scene (ten tries,
validity test, the last try when none is valid) and draws npoints of its points with
replacement. Here the whole sampler runs on the GPU (csrc/scene.hip: pn2_scene_bbox,
pn2_crop_sample), for a batch of crops of one scene at once. The reference draws its random
numbers with tf.random_uniform; here the draws are explicit inputs (centres, u) or taken from a
torch.Generator, and for the same draws the result is the reference's.

Reference quirk kept: the validity test divides the labelled-point count by
reduce_sum(ones_like(cur_points)) = 3 n (the (n, 3) tensor, :113), so no try is ever valid and
every crop is the LAST try's column.

label_map, label_map_numpy and label_map_more_parameters (:25-67) map a scene's NYU-40 label ids
to 0..20 through torch.ops.pn2.label_lut (csrc/predict.hip), the look-up kernel that
generate_predictions.map_to_nyu40 and evaluate.evaluate_scan share.

random_rotate (:334-352), the reference's only augmentation, and the validation chunker
get_all_subsets_for_scene_numpy (:270-331, every validation batch of precompute_val_data) run on
csrc/feed.hip and pn2_val_select: torch.ops.pn2.feed_batch, val_select and val_chunks, which have
CUDA kernels and host twins with equal bits, so the functions below take tensors of either
device. scene_val_chunks is the chunker with device tensors in and out.
"""
import math

import numpy as np
import torch

from . import _torch_ops
from ._lib import InvalidArgumentError, check, device_tensor, lib, ptr, stream_of

LABEL_WEIGHTS = [0, 2.743064592944318, 3.0830506790927132, 4.785754459526457, 4.9963745147506184,
                 4.372710774561782, 5.039124880965811, 4.86451825464344, 4.717751595568025,
                 4.809412839311939, 5.052097251455304, 5.389129668645318, 5.390614085649042,
                 5.127458225110977, 5.086056870814752, 5.3831185190895265, 5.422684124268539,
                 5.422955391988761, 5.433705358072363, 5.417426773812747,
                 4.870172044153657]  # data_transformation.py:82-86
TRIES = 10  # :138-141
# :21-22, the NYU-40 ids of the 20 ScanNet classes -> 1..20; every other id -> 0
LABEL_MAP = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10, 11: 11, 12: 12, 14: 13,
             16: 14, 24: 15, 28: 16, 33: 17, 34: 18, 36: 19, 39: 20}
LABEL_LUT = [LABEL_MAP.get(i, 0) for i in range(41)]  # :36, :53


def _label_lut(labels):
    """LABEL_LUT over int32 labels on their device (torch.ops.pn2.label_lut; CPU tensors run the
    host twin). A label past 40 gives 0, which is the reference's map[min(label, 40)]; a negative
    label gives 0 too, where the reference's gather wraps around (numpy) or raises (TF)."""
    lut = torch.tensor(LABEL_LUT, dtype=torch.int32, device=labels.device)
    return _torch_ops.call("label_lut", labels.to(torch.int32), lut, 0)


def label_map(points, labels, colors, normals):
    """:25-39: the labels of a scene from NYU-40 ids to 0..20, tensors (the TF function);
    points, colors and normals pass through. Returns (points, mapped labels int32, colors,
    normals)."""
    return points, _label_lut(labels), colors, normals


def label_map_numpy(points, labels, colors, normals):
    """:42-56: label_map on numpy arrays; the mapped labels are int64 as the reference's
    np.array of Python ints."""
    mapped = label_map_more_parameters(labels)
    return points, mapped, colors, normals


def label_map_more_parameters(labels):
    """:59-67: LABEL_MAP.get(label, 0) over an array of labels, int64."""
    a = np.asarray(labels)
    t = torch.from_numpy(np.ascontiguousarray(np.clip(a, -1, 2 ** 31 - 1).astype(np.int32)))
    return _label_lut(t).numpy().astype(np.int64).reshape(a.shape)


def scene_bbox(points):
    """[min xyz, max xyz] of a (N,3) scene on the GPU (reduce_min / reduce_max, :90-91)."""
    points = device_tensor(points, "points", torch.float32)
    N = int(points.shape[0])
    ws = torch.empty(int(lib().pn2_scene_workspace_size(N)) // 4 + 1, dtype=torch.float32,
                     device=points.device)
    bbox = torch.empty(6, dtype=torch.float32, device=points.device)
    check(lib().pn2_scene_bbox(ptr(points), N, ptr(bbox), ptr(ws), ws.numel() * 4,
                               stream_of(points)), "scene_bbox")
    return bbox


def get_subsets(points, labels, colors, normals, batch, npoints=8192, centres=None, u=None,
                generator=None, label_weights=None, bbox=None):
    """`batch` crops of one scene: get_subset (:70-154) batched. centres (batch, TRIES) int32
    point indices and u (batch, npoints) uniform draws default to draws from `generator`
    (the reference's tf.random_uniform((1,), 0, len) and ((npoints,), 0, cur_len)).
    Returns points (batch,npoints,3), labels (batch,npoints), colors (batch,npoints,3) int32,
    normals (batch,npoints,3), sample_weights (batch,npoints); colors / normals may be None."""
    points = device_tensor(points, "points", torch.float32)
    labels = device_tensor(labels, "labels", torch.int32)
    dev = points.device
    N = int(points.shape[0])
    if points.dim() != 2 or points.shape[1] != 3 or tuple(labels.shape) != (N,):
        raise InvalidArgumentError("get_subset expects points (N,3) and labels (N)")
    colors = None if colors is None else device_tensor(colors, "colors", torch.int32)
    normals = None if normals is None else device_tensor(normals, "normals", torch.float32)
    if centres is None:
        r = torch.rand((batch, TRIES), generator=generator, device=dev)
        centres = (r * float(N)).to(torch.int32).clamp_(0, N - 1)
    if u is None:
        u = torch.rand((batch, npoints), generator=generator, device=dev)
    # the draws may come from the host (numpy / CPU tensors): they are inputs, not compute
    centres = device_tensor(torch.as_tensor(centres).to(dev), "centres", torch.int32)
    u = device_tensor(torch.as_tensor(u).to(dev), "u", torch.float32)
    T = int(centres.shape[1])
    lw = torch.tensor(LABEL_WEIGHTS if label_weights is None else label_weights,
                      dtype=torch.float32, device=dev)
    if bbox is None:
        bbox = scene_bbox(points)
    ws = torch.empty(int(lib().pn2_crop_workspace_size(batch, N, T)) // 4 + 1,
                     dtype=torch.float32, device=dev)
    op = torch.empty((batch, npoints, 3), dtype=torch.float32, device=dev)
    ol = torch.empty((batch, npoints), dtype=torch.int32, device=dev)
    oc = None if colors is None else torch.empty((batch, npoints, 3), dtype=torch.int32, device=dev)
    on = None if normals is None else torch.empty((batch, npoints, 3), dtype=torch.float32,
                                                  device=dev)
    ow = torch.empty((batch, npoints), dtype=torch.float32, device=dev)
    check(lib().pn2_crop_sample(ptr(points), ptr(labels), ptr(colors), ptr(normals), N, ptr(bbox),
                                ptr(centres), batch, T, ptr(u), npoints, ptr(lw), lw.numel(),
                                ptr(ws), ws.numel() * 4, ptr(op), ptr(ol), ptr(oc), ptr(on),
                                ptr(ow), stream_of(points)), "get_subset")
    return op, ol, oc, on, ow


def get_subset(points, labels, colors, normals, npoints=8192, centres=None, u=None,
               generator=None):
    """data_transformation.py:70-154 for one crop: (points (K,3), labels (K), colors (K,3),
    normals (K,3), sample_weights (K))."""
    if centres is not None:
        centres = torch.as_tensor(centres).reshape(1, -1)
    if u is not None:
        u = torch.as_tensor(u).reshape(1, -1)
    outs = get_subsets(points, labels, colors, normals, 1, npoints, centres, u, generator)
    return tuple(None if o is None else o[0] for o in outs)


def rotation_cs(alpha):
    """(cos alpha, sin alpha) as float32, the pair random_rotate hands to the kernel; the device
    never computes them. alpha is rounded to float32 first (TF's alpha is a float32 scalar,
    :347), its cosine and sine are taken by the host's libm in double and rounded to float32
    once. alpha: a number or a (B,) sequence; returns a float32 array (2,) or (B, 2)."""
    a = np.asarray(alpha, dtype=np.float32).astype(np.float64)
    cs = np.stack([np.cos(a), np.sin(a)], axis=-1)
    return cs.astype(np.float32)


def _empty_weights(dev):
    return torch.empty(0, dtype=torch.float32, device=dev)


def random_rotate(points, labels, colors, normals, sample_weight, alpha=None, generator=None):
    """:334-352: the cloud rotated about z by alpha, points and normals; labels, colors and
    sample_weight pass through. points (N,3) or (B,N,3) float32 on the GPU (or the CPU: the host
    twin, equal bits), normals likewise or None. alpha: one angle, or one per cloud (B,); None
    draws each cloud's angle uniformly in [0, 2 pi) from `generator` (torch's CPU generator),
    the reference's tf.random_uniform([], 0, 2 pi). One torch.ops.pn2.feed_batch launch:
    x' = x c + y s, y' = y c - x s with (c, s) = rotation_cs(alpha), each product rounded, then
    the sum (the row vector times [[c,-s,0],[s,c,0],[0,0,1]], :348-351).
    Returns (rot_points, labels, colors, rot_normals, sample_weight)."""
    if not isinstance(points, torch.Tensor) or points.dtype != torch.float32:
        raise TypeError("random_rotate expects float32 tensor points")
    single = points.dim() == 2
    P = points.unsqueeze(0) if single else points
    if P.dim() != 3 or P.shape[2] != 3:
        raise InvalidArgumentError("random_rotate expects points (N,3) or (B,N,3)")
    B, N = int(P.shape[0]), int(P.shape[1])
    dev = P.device
    if alpha is None:
        alpha = (torch.rand(B, generator=generator, dtype=torch.float64) * (2 * math.pi)).numpy()
    cs = rotation_cs(np.broadcast_to(np.asarray(alpha, dtype=np.float64).reshape(-1), (B,)))
    nrm = None
    if normals is not None:
        nrm = normals.unsqueeze(0) if single else normals
    zeros_i = torch.zeros((B, N), dtype=torch.int32, device=dev)
    zeros_f = torch.zeros((B, N), dtype=torch.float32, device=dev)
    xyz, feats, _ = _torch_ops.call("feed_batch", P, zeros_i, None, nrm, zeros_f,
                                    torch.from_numpy(cs).to(dev), _empty_weights(dev), False,
                                    nrm is not None)
    rot_normals = None if nrm is None else feats
    if single:
        xyz = xyz[0]
        rot_normals = None if rot_normals is None else rot_normals[0]
    return xyz, labels, colors, rot_normals, sample_weight


VAL_MARGIN = 0.2          # :302, the selection margin of a column
VAL_INNER_MARGIN = 0.001  # :309, the mask's margin
VAL_MIN_INSIDE = 0.01     # :317


def _as_scene(points, labels, colors, normals, device):
    """The scene's arrays as contiguous tensors on `device`: float32 points and normals, int32
    labels and colours."""
    def conv(a, dtype):
        if a is None:
            return None
        t = torch.as_tensor(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        return t.to(device=device, dtype=dtype).contiguous()
    P = conv(points, torch.float32)
    if P.dim() != 2 or P.shape[1] != 3:
        raise InvalidArgumentError("the validation chunker expects points (N,3)")
    return P, conv(labels, torch.int32), conv(colors, torch.int32), conv(normals, torch.float32)


def _val_bounds(P):
    """The (S, 6) float64 column bounds of :289-301, built on the host exactly as the reference
    builds them, from one read of the scene's bounding box (reduce_min / reduce_max are exact)."""
    if P.shape[0] == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    if P.device.type == "cuda":
        bbox = scene_bbox(P).cpu().numpy()
    else:
        bbox = torch.cat([P.amin(dim=0), P.amax(dim=0)]).numpy()
    coordmin, coordmax = bbox[:3], bbox[3:]
    nsubvolume_x = np.ceil((coordmax[0] - coordmin[0]) / 1.5).astype(np.int32)
    nsubvolume_y = np.ceil((coordmax[1] - coordmin[1]) / 1.5).astype(np.int32)
    bounds = []
    for i in range(nsubvolume_x):
        for j in range(nsubvolume_y):
            curmin = coordmin + [i * 1.5, j * 1.5, 0]  # float64 (:300-301)
            curmax = coordmin + [(i + 1) * 1.5, (j + 1) * 1.5, coordmax[2] - coordmin[2]]
            bounds.append(np.concatenate([curmin, curmax]))
    return np.asarray(bounds, np.float64).reshape(-1, 6)


def _val_label_weights(dev):
    w = torch.ones(21, dtype=torch.float32, device=dev)  # :286-287
    w[0] = 0
    return w


def scene_val_chunks(points, labels, colors, normals, npoints=8192, choice=None, u=None,
                     generator=None, device=None):
    """The validation chunks of one scene (get_all_subsets_for_scene_numpy, :270-331) as device
    tensors: the scene is cut into 1.5 m x 1.5 m columns (0.2 m margin); every non-empty column
    gives one chunk of npoints draws with replacement, mask = inside the column + 0.001,
    weight = (label != 0) * mask, and a chunk with less than 1 % of its draws inside is dropped.
    Selection, draws, the keep test, the compaction and the gathers run on the device
    (torch.ops.pn2.val_select, val_chunks; csrc/scene.hip, csrc/feed.hip).

    choice (S, npoints) int32: the draws of every column in column order (i outer, j inner);
    else u (S, npoints) uniform [0, 1) draws, index = int(u * n) as in get_subset; else u is
    drawn from `generator` on the points' device. The host reads the bounding box (to lay out
    the columns) and `kept` (to slice the padded outputs), nothing else.
    Returns (points (X,npoints,3), labels (X,npoints) int32, colors (X,npoints,3) int32 or None,
    normals (X,npoints,3) or None, weights (X,npoints) float32); X may be 0.

    Not the TF function get_all_subsets_for_scene (:157-267): its validity test divides the
    labelled count by 3 n, like get_subset's, never passes, and so it returns no chunk at all;
    that name is left unused on purpose."""
    dev = torch.device(device) if device is not None else (
        points.device if isinstance(points, torch.Tensor) else torch.device("cuda"))
    P, L, C, Nn = _as_scene(points, labels, colors, normals, dev)
    if npoints < 0:
        raise InvalidArgumentError("scene_val_chunks expects npoints >= 0")
    bounds = torch.from_numpy(_val_bounds(P)).to(dev)
    S = int(bounds.shape[0])
    counts, sel, inner = _torch_ops.call("val_select", P, bounds, VAL_MARGIN, VAL_INNER_MARGIN)
    if choice is not None:
        choice = torch.as_tensor(choice).to(device=dev, dtype=torch.int32).reshape(S, npoints)
    elif u is not None:
        u = torch.as_tensor(u).to(device=dev, dtype=torch.float32).reshape(S, npoints)
    else:
        u = torch.rand((S, npoints), generator=generator, device=dev)
    op, ol, oc, on, ow, _, kept = _torch_ops.call(
        "val_chunks", P, L, C, Nn, counts, sel, inner, choice, u, npoints,
        _val_label_weights(dev), VAL_MIN_INSIDE)
    X = int(kept.item())
    return (op[:X], ol[:X], None if C is None else oc[:X], None if Nn is None else on[:X],
            ow[:X])


def get_all_subsets_for_scene_numpy(points, labels, colors, normals, npoints=8192, device="cuda"):
    """:270-331 with the reference's numpy interface: (points (X,K,3) float32, labels (X,K) in
    the labels' dtype, colors (X,K,3) int32, normals (X,K,3) float32, sample_weights (X,K)
    float64). The reference's only random call, np.random.choice(n, npoints, replace=True) per
    non-empty column in column order, is made here on the host from the counts (read back
    once), so under the same np.random.seed the output is the reference's bit for bit; the rest
    is scene_val_chunks. A column whose chunk is dropped has still been drawn for. When every
    column is skipped the reference's np.concatenate of nothing raises ValueError; so does
    this."""
    dev = torch.device(device)
    P, L, C, Nn = _as_scene(points, labels, colors, normals, dev)
    if npoints < 0:
        raise ValueError("negative dimensions are not allowed")  # np.random.choice's
    bounds = torch.from_numpy(_val_bounds(P)).to(dev)
    S = int(bounds.shape[0])
    counts, sel, inner = _torch_ops.call("val_select", P, bounds, VAL_MARGIN, VAL_INNER_MARGIN)
    choice = np.zeros((S, npoints), np.int32)
    for s, n in enumerate(counts.cpu().numpy()):
        if n:  # :307-308: an empty column draws nothing
            choice[s] = np.random.choice(int(n), npoints, replace=True)  # :311
    op, ol, oc, on, ow, _, kept = _torch_ops.call(
        "val_chunks", P, L, C, Nn, counts, sel, inner, torch.from_numpy(choice).to(dev), None,
        npoints, _val_label_weights(dev), VAL_MIN_INSIDE)
    X = int(kept.item())
    if X == 0:
        raise ValueError("need at least one array to concatenate")
    ldt = labels.dtype if isinstance(labels, np.ndarray) else np.int32
    return (op[:X].cpu().numpy(), ol[:X].cpu().numpy().astype(ldt, copy=False),
            None if C is None else oc[:X].cpu().numpy(),
            None if Nn is None else on[:X].cpu().numpy(),
            ow[:X].cpu().numpy().astype(np.float64))
