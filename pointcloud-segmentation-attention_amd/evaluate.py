"""attention_points/benchmark/evaluate.py: the ScanNet benchmark's score of predicted NYU-40 ids.

The reference loops over the points in Python (:78-83): a ground-truth id outside
VALID_CLASS_IDS is skipped, a prediction outside it counts in column UNKNOWN_ID = 40 of a
41 x 41 confusion matrix. Here the two membership tests are table look-ups
(torch.ops.pn2.label_lut: ground truth not valid -> 0, prediction not valid -> 40) and the
counting is torch.ops.pn2.seg_confusion with C = 41, whose rule 0 < label < C, 0 <= pred < C is
exactly the reference's: the matrix is an int64 (41, 41) tensor on the device and a scene's ids
are read once. get_iou and write_result_file work on the integers, on the host.

A CPU confusion tensor is accepted too (the host twins pn2cpu_label_lut and
pn2cpu_seg_confusion: equal integers), so scores can be computed and tested without a GPU.
"""
import sys

import numpy as np
import torch

from . import _torch_ops
from ._lib import check, lib

CLASS_LABELS = ['wall', 'floor', 'cabinet', 'bed', 'chair', 'sofa', 'table', 'door', 'window',
                'bookshelf', 'picture', 'counter', 'desk', 'curtain', 'refrigerator',
                'shower curtain', 'toilet', 'sink', 'bathtub', 'otherfurniture']  # :51-53
VALID_CLASS_IDS = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39])
UNKNOWN_ID = np.max(VALID_CLASS_IDS) + 1  # 40

_N = int(UNKNOWN_ID) + 1
_VALID = set(int(v) for v in VALID_CLASS_IDS)
GT_LUT = [i if i in _VALID else 0 for i in range(_N)]                  # not valid: skipped
PRED_LUT = [i if i in _VALID else int(UNKNOWN_ID) for i in range(_N)]  # not valid: unknown


def load_ids(filename):
    """:39-48: the ids of a file with one id per line, int64."""
    ids = open(filename).read().splitlines()
    ids = np.array(ids, dtype=np.int64)
    return ids


def _ids(x, device):
    """File name, array or tensor -> flat int32 tensor on `device` (ids outside int32 are no
    class: -1)."""
    if isinstance(x, str):
        x = load_ids(x)
    if isinstance(x, torch.Tensor):
        return x.reshape(-1).to(device).clamp(-1, 2 ** 31 - 1).to(torch.int32)
    x = np.asarray(x).reshape(-1)
    x = np.clip(np.nan_to_num(x.astype(np.float64), nan=-1.0), -1, 2 ** 31 - 1)
    return torch.from_numpy(x.astype(np.int32)).to(device)


def new_confusion(device="cuda"):
    """The zeroed (41, 41) int64 confusion matrix evaluate() accumulates into."""
    return torch.zeros((_N, _N), dtype=torch.int64, device=device)


def evaluate_scan(pred, gt, confusion):
    """:58-83: adds one scene to `confusion`, an int64 (41, 41) tensor (rows: ground truth,
    columns: prediction, NYU-40 ids), in place. pred / gt: file names (load_ids), arrays or
    tensors of ids. Points whose ground truth is not in VALID_CLASS_IDS are skipped; a prediction
    not in VALID_CLASS_IDS counts in column UNKNOWN_ID."""
    dev = confusion.device
    pred_ids, gt_ids = _ids(pred, dev), _ids(gt, dev)
    if pred_ids.shape != gt_ids.shape:  # :76-77 prints and goes on to zip(): the common prefix
        print('%s: number of predicted values does not match number of vertices' % (pred,))
        n = min(pred_ids.numel(), gt_ids.numel())
        pred_ids, gt_ids = pred_ids[:n], gt_ids[:n]
    lut = lambda t: torch.tensor(t, dtype=torch.int32, device=dev)  # noqa: E731
    gt_m = _torch_ops.call("label_lut", gt_ids, lut(GT_LUT), 0)
    pred_m = _torch_ops.call("label_lut", pred_ids, lut(PRED_LUT), int(UNKNOWN_ID))
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    if dev.type == "cpu":
        if confusion.dtype != torch.int64 or tuple(confusion.shape) != (_N, _N) or \
                not confusion.is_contiguous():
            raise ValueError("evaluate_scan expects a contiguous int64 (41, 41) confusion")
        check(lib().pn2cpu_seg_confusion(gt_m.data_ptr(), pred_m.data_ptr(), gt_m.numel(), _N,
                                         confusion.data_ptr(), counts.data_ptr()),
              "seg_confusion")
    else:
        _torch_ops.call("seg_confusion", gt_m, pred_m, confusion, counts)


def get_iou(label_id, confusion):
    """:86-108: (tp / (tp + fp + fn), tp, tp + fp + fn) of an NYU-40 id from the confusion
    matrix (tensor or array), computed on the host from the integers; NaN for an id outside
    VALID_CLASS_IDS or one that occurs neither as ground truth nor as a prediction. fn counts the
    UNKNOWN_ID column, fp only the rows of the other valid ids."""
    if int(label_id) not in _VALID:
        return float('nan')
    cm = confusion.cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
    label_id = int(label_id)
    tp = int(cm[label_id, label_id])
    fn = int(cm[label_id, :].sum()) - tp
    not_ignored = [int(l) for l in VALID_CLASS_IDS if not l == label_id]
    fp = int(cm[not_ignored, label_id].sum())
    denom = tp + fp + fn
    if denom == 0:
        return float('nan')
    return (float(tp) / denom, tp, denom)


def write_result_file(confusion, ious, filename):
    """:111-138, the reference's text: the IoU per class, then the confusion matrix over the
    valid ids. ious: {class name: get_iou's value}; a NaN (a class that never occurs, where the
    reference raises TypeError) is written as nan."""
    cm = confusion.cpu().numpy() if isinstance(confusion, torch.Tensor) else np.asarray(confusion)
    with open(filename, 'w') as f:
        f.write('iou scores\n')
        for i in range(len(VALID_CLASS_IDS)):
            label_id = int(VALID_CLASS_IDS[i])
            label_name = CLASS_LABELS[i]
            v = ious[label_name]
            iou = v[0] if isinstance(v, tuple) else v
            f.write('{0:<14s}({1:<2d}): {2:>5.3f}\n'.format(label_name, label_id, iou))
        f.write('\nconfusion matrix\n')
        f.write('\t\t\t')
        for i in range(len(VALID_CLASS_IDS)):
            f.write('{0:<8d}'.format(int(VALID_CLASS_IDS[i])))
        f.write('\n')
        for r in range(len(VALID_CLASS_IDS)):
            f.write('{0:<14s}({1:<2d})'.format(CLASS_LABELS[r], int(VALID_CLASS_IDS[r])))
            for c in range(len(VALID_CLASS_IDS)):
                f.write('\t{0:>5.3f}'.format(int(cm[VALID_CLASS_IDS[r], VALID_CLASS_IDS[c]])))
            f.write('\n')
    print('wrote results to', filename)


def evaluate(pred_files, gt_files, output_file_path, device="cuda"):
    """:141-171: the confusion matrix over all scenes, the IoU of every class, the summary on
    stdout and the result file. pred_files / gt_files: file names (or arrays). Returns
    (confusion, {class name: get_iou's value})."""
    confusion = new_confusion(device)
    print('evaluating', len(pred_files), 'scans...')
    for i in range(len(pred_files)):
        evaluate_scan(pred_files[i], gt_files[i], confusion)
        sys.stdout.write("\rscans processed: {}".format(i + 1))
        sys.stdout.flush()
    print('')
    cm = confusion.cpu().numpy()
    class_ious = {}
    for i in range(len(VALID_CLASS_IDS)):
        class_ious[CLASS_LABELS[i]] = get_iou(VALID_CLASS_IDS[i], cm)
    print('classes          IoU')
    print('----------------------------')
    for i in range(len(VALID_CLASS_IDS)):
        v = class_ious[CLASS_LABELS[i]]
        if isinstance(v, tuple):
            print('{0:<14s}: {1:>5.3f}   ({2:>6d}/{3:<6d})'.format(CLASS_LABELS[i], v[0], v[1], v[2]))
        else:
            print('{0:<14s}:   nan'.format(CLASS_LABELS[i]))
    write_result_file(cm, class_ious, output_file_path)
    return confusion, class_ious
