"""attention_points/train.py: what the reference's training loop (:288-387) runs around the
model, on the gfx950 kernels of csrc/optim.hip.

    get_learning_rate, get_bn_decay   the two staircase schedules (:27-58), Python floats
    AdamOptimizer                     tf.train.AdamOptimizer (:337): TF 1.x ApplyAdam over every
                                      variable in ceil(n / 64) launches (torch.ops.pn2.adam_step)
    SegMetrics                        get_metrics (:145-163): the accuracy over the annotated
                                      points and the streaming tf.metrics.mean_iou
    train_step, train_step_with       one step: forward, weighted loss, backward, Adam, metrics
                                      (train_step_with takes the model: the attention models)
    eval_step                         one validation batch (eval_model, :221-285): the inference
                                      path, the same loss and metrics, nothing updated
    CLASS_WEIGHTS, get_data_tensors   a stored batch as model inputs (:74-109) in one launch
                                      (torch.ops.pn2.feed_batch, csrc/feed.hip)
    choose_model, eval_model, train   the model choice (:291-293, :323-330), the validation pass
                                      (:221-285) and the epoch loop (:288-387)

A loop written against this module never reads the device back inside a step:

    store = tf_util.ParamStore(seed=0).trainable("cuda")
    opt, metrics = AdamOptimizer(store), SegMetrics(21)
    for batch, (xyz, feats, labels, smpw) in enumerate(loader):
        loss, counts = train_step(store, opt, metrics, xyz, labels, smpw, 21,
                                  bn_decay=get_bn_decay(batch),
                                  learning_rate=get_learning_rate(batch), features=feats)
    mean_iou, per_class = metrics.iou()
"""
import math
import os

import numpy as np
import torch

from . import _torch_ops, pointnet2_sem_seg_attention, pointnet2_sem_seg_attention_single_layer
from .data_transformation import LABEL_WEIGHTS
from .pointnet2_sem_seg import model_body
from .tf_util import ParamStore

BATCH_SIZE = 16         # train.py:17
N_TRAIN_SAMPLES = 1201  # train.py:15, the number of train scenes
DECAY_EPOCHS = 80       # train.py:37, :54: decay_steps = N_TRAIN_SAMPLES * 80
CLASS_WEIGHTS = list(LABEL_WEIGHTS)  # train.py:20-24, the table of data_transformation.py:82-86


def _staircase(batch, batch_size, n_train_samples):
    """tf.train.exponential_decay's exponent with staircase=True."""
    return (int(batch) * int(batch_size)) // (int(n_train_samples) * DECAY_EPOCHS)


def get_learning_rate(batch, batch_size=BATCH_SIZE, n_train_samples=N_TRAIN_SAMPLES):
    """train.py:27-41: 1e-3 * 0.7 ** k with k = (batch * batch_size) // (n_train_samples * 80),
    clipped from below at 1e-5."""
    return max(1e-3 * 0.7 ** _staircase(batch, batch_size, n_train_samples), 1e-5)


def get_bn_decay(batch, batch_size=BATCH_SIZE, n_train_samples=N_TRAIN_SAMPLES):
    """train.py:44-58: min(0.99, 1 - 0.5 * 0.5 ** k) with get_learning_rate's k."""
    return min(0.99, 1 - 0.5 * 0.5 ** _staircase(batch, batch_size, n_train_samples))


class AdamOptimizer:
    """tf.train.AdamOptimizer(learning_rate, beta1, beta2, epsilon) on torch.ops.pn2.adam_step
    (csrc/optim.hip: TF 1.x ApplyAdam without Nesterov).

    `params`: an iterable of leaves (store.parameters()) or a tf_util.ParamStore. Given a store,
    the slot variables carry the reference's names (<var>/Adam, <var>/Adam_1) and a variable the
    model creates after construction is picked up at the next step() with zero slots.

    step() folds both bias corrections into the step size, alpha = lr * sqrt(1 - beta2^t) /
    (1 - beta1^t), and adds epsilon to the uncorrected sqrt(v): TF's update, not torch.optim.Adam's,
    which divides sqrt(v) by sqrt(1 - beta2^t) before it adds epsilon. The trajectory's bits are
    this package's, not TensorFlow's, for two reasons: TF keeps beta1_power and beta2_power as
    fp32 variables multiplied once per step and computes alpha from them in fp32, while here
    alpha comes from t in double (beta1 and beta2 rounded to fp32 first, alpha rounded to fp32
    last); and TF's kernels may contract the update's multiplies and adds, while every operation
    here rounds on its own (the host twin pn2cpu_adam_step pins the bits)."""

    def __init__(self, params, learning_rate=1e-3, beta1=0.9, beta2=0.999, epsilon=1e-8):
        self.learning_rate = float(learning_rate)
        self.beta1 = float(np.float32(beta1))
        self.beta2 = float(np.float32(beta2))
        self.epsilon = float(epsilon)
        if not (0.0 <= self.beta1 < 1.0 and 0.0 <= self.beta2 < 1.0 and self.epsilon >= 0.0):
            raise ValueError("AdamOptimizer expects beta1 and beta2 in [0, 1) and epsilon >= 0")
        self.t = 0
        self.store = params if isinstance(params, ParamStore) else None
        self._leaves = None if self.store is not None else list(params)
        self._slots = {}    # name -> (exp_avg, exp_avg_sq)
        self._loaded = {}   # slots of load_state_dict whose variable does not exist yet

    def named_parameters(self):
        """(name, leaf) of every trainable variable: the store's TF names, or the position in
        the list the optimiser was built from."""
        if self.store is not None:
            return [(k, v) for k, v in self.store.items() if v.requires_grad]
        return [(str(i), p) for i, p in enumerate(self._leaves)]

    def _slot(self, name, p):
        """The slot variables of `name`: loaded ones, or zeros (TF's slot initialiser)."""
        hit = self._slots.get(name)
        if hit is None or hit[0].shape != p.shape or hit[0].device != p.device:
            loaded = self._loaded.pop(name, None)
            if loaded is not None:
                hit = tuple(torch.as_tensor(a, dtype=torch.float32).reshape(p.shape).to(
                    p.device, copy=True).contiguous() for a in loaded)
            else:
                hit = (torch.zeros_like(p, memory_format=torch.contiguous_format),
                       torch.zeros_like(p, memory_format=torch.contiguous_format))
            self._slots[name] = hit
        return hit

    def zero_grad(self):
        """Gradients to None (torch's set_to_none)."""
        for _, p in self.named_parameters():
            p.grad = None

    def alpha(self, learning_rate=None):
        """The step size of step number self.t, rounded to fp32."""
        lr = self.learning_rate if learning_rate is None else float(learning_rate)
        return float(np.float32(lr * math.sqrt(1.0 - self.beta2 ** self.t)
                                / (1.0 - self.beta1 ** self.t)))

    @torch.no_grad()
    def step(self, learning_rate=None):
        """One ApplyAdam over every parameter whose .grad is not None, in one adam_step call;
        the others and their slots stay untouched. `learning_rate` overrides the constructor's
        for this step (the schedule's value). Nothing synchronises."""
        self.t += 1
        params, grads, ms, vs = [], [], [], []
        for name, p in self.named_parameters():
            if p.grad is None:
                continue
            m, v = self._slot(name, p)
            params.append(p)
            grads.append(p.grad.contiguous())
            ms.append(m)
            vs.append(v)
        if params:
            _torch_ops.call("adam_step", params, grads, ms, vs, self.alpha(learning_rate),
                            self.beta1, self.beta2, self.epsilon)

    def state_dict(self):
        """CPU float32 arrays under the reference checkpoint's names: <var>/Adam and
        <var>/Adam_1 for every variable, beta1_power, beta2_power (beta ** t) and global_step."""
        d = {}
        for name, p in self.named_parameters():
            m, v = self._slot(name, p)
            d[f"{name}/Adam"] = m.detach().cpu().numpy().copy()
            d[f"{name}/Adam_1"] = v.detach().cpu().numpy().copy()
        for name, (m, v) in self._loaded.items():
            d[f"{name}/Adam"] = np.array(m, dtype=np.float32)
            d[f"{name}/Adam_1"] = np.array(v, dtype=np.float32)
        d["beta1_power"] = np.float32(self.beta1 ** self.t)
        d["beta2_power"] = np.float32(self.beta2 ** self.t)
        d["global_step"] = np.int64(self.t)
        return d

    def load_state_dict(self, d):
        """Restore state_dict()'s arrays (or a reference checkpoint's Adam variables, exported to
        a dict). t is global_step; the beta powers are not read (they follow from t). Slots of
        variables that do not exist yet wait until the model creates them."""
        self.t = int(np.asarray(d["global_step"]))
        self._slots.clear()
        self._loaded = {}
        for key in d:
            if key.endswith("/Adam"):
                name = key[:-len("/Adam")]
                if f"{name}/Adam_1" not in d:
                    raise KeyError(f"{name}/Adam_1")
                self._loaded[name] = (np.asarray(d[key], dtype=np.float32),
                                      np.asarray(d[f"{name}/Adam_1"], dtype=np.float32))
        for name, p in self.named_parameters():
            if name in self._loaded:
                self._slot(name, p)


class SegMetrics:
    """get_metrics' accuracy and mean IoU (train.py:145-163) on torch.ops.pn2.seg_confusion and
    mean_iou: an int64 (C, C) confusion matrix on the device, accumulated over update() calls
    like tf.metrics.mean_iou's total_cm. Points with label 0 (unannotated) are left out."""

    def __init__(self, num_classes, device="cuda"):
        self.num_classes = int(num_classes)
        self.confusion = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64,
                                     device=device)

    def update(self, labels, pred):
        """Add a batch: labels (...) integer, pred (...) int32 (softmax_xent's argmax). Returns
        this batch's counts = (correct, assigned) as an int64 device tensor; no
        synchronisation."""
        if labels.dtype in (torch.int64, torch.int16, torch.uint8, torch.int8):
            labels = labels.to(torch.int32)
        counts = torch.zeros(2, dtype=torch.int64, device=self.confusion.device)
        _torch_ops.call("seg_confusion", labels, pred, self.confusion, counts)
        return counts

    @staticmethod
    def accuracy(counts):
        """correct / assigned of update()'s counts as a float (reads the device); NaN when
        nothing is assigned, TensorFlow's 0 / 0."""
        correct, assigned = (int(c) for c in counts.tolist())
        return correct / assigned if assigned else float("nan")

    def iou(self):
        """(mean IoU, per-class IoU (C,)) of everything added since reset(), float32 device
        tensors: tf.metrics.mean_iou's value. Classes that occur neither as a label nor as a
        prediction are left out of the mean and read 0 per class."""
        return tuple(_torch_ops.call("mean_iou", self.confusion))

    def reset(self):
        self.confusion.zero_()


def train_step_with(model, store, opt, metrics, point_cloud, labels, smpw, num_class,
                    bn_decay=None, learning_rate=None, features=None, seed=None):
    """One training step of train.py's loop on a trainable store with `model`, a callable with
    pointnet2_sem_seg.model_body's signature (the attention models' `body`; None: model_body
    itself): zero_grad, the model with is_training=True, the weighted loss, backward,
    opt.step(learning_rate), metrics.update with the loss kernel's own argmax (no second pass
    over the logits). `seed`: the dropout seed, so a step is reproducible. Returns (loss,
    counts), device tensors: nothing here reads the device back."""
    opt.zero_grad()
    body = model_body if model is None else model
    logits, _ = body(point_cloud, features, True, num_class, bn_decay, store, seed=seed)
    if labels.dtype in (torch.int64, torch.int16, torch.uint8, torch.int8):
        labels = labels.to(torch.int32)
    loss, _, pred, _ = _torch_ops.call("softmax_xent", logits, labels, smpw)
    loss.backward()
    opt.step(learning_rate)
    counts = metrics.update(labels, pred)
    return loss.detach(), counts


def train_step(store, opt, metrics, point_cloud, labels, smpw, num_class, bn_decay=None,
               learning_rate=None, features=None, seed=None):
    """train_step_with on pointnet2_sem_seg.model_body: pointnet2_sem_seg, or
    pointnet2_sem_seg_features when `features` (B, N, C) is given. Its parameter list is kept as
    it was; the attention models train through train_step_with(model, ...)."""
    return train_step_with(None, store, opt, metrics, point_cloud, labels, smpw, num_class,
                           bn_decay, learning_rate, features, seed)


@torch.no_grad()
def eval_step(store, metrics, point_cloud, labels, smpw, num_class, features=None, model=None):
    """One batch of train.py's validation pass (eval_model, :221-285): train_step without
    zero_grad, backward and the optimiser, with is_training=False, so the model runs its inference
    path on the moving statistics and no variable of the store changes. The weighted loss and the
    metrics are train_step's: softmax_xent's loss and argmax, metrics.update. `model`: as in
    train_step. Returns (loss, counts), device tensors: nothing here reads the device back."""
    body = model_body if model is None else model
    logits, _ = body(point_cloud, features, False, num_class, None, store)
    if labels.dtype in (torch.int64, torch.int16, torch.uint8, torch.int8):
        labels = labels.to(torch.int32)
    loss, _, pred, _ = _torch_ops.call("softmax_xent", logits, labels, smpw)
    counts = metrics.update(labels, pred)
    return loss, counts


def get_data_tensors(batch, color=True, normal=True, device="cuda"):
    """train.py:74-109 for one stored batch = (points (B,N,3) float32, labels (B,N), colors
    (B,N,3) integers, normals (B,N,3) float32, sample_weight (B,N)), numpy or tensors:
    colors / 255, features = colors ++ normals (either alone, or None), and sample_weight =
    CLASS_WEIGHTS[labels] * (stored weight != 0), in ONE launch (torch.ops.pn2.feed_batch;
    csrc/feed.hip) instead of eight. Returns (xyz, labels int32, features or None, smpw) on
    `device`."""
    dev = torch.device(device)

    def conv(a, dtype):
        if a is None:
            return None
        t = torch.as_tensor(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        return t.to(device=dev, dtype=dtype)
    points, labels, colors, normals, weight = batch
    points, labels = conv(points, torch.float32), conv(labels, torch.int32)
    colors = conv(colors, torch.int32) if color else None
    normals = conv(normals, torch.float32) if normal else None
    cw = torch.tensor(CLASS_WEIGHTS, dtype=torch.float32, device=dev)
    xyz, feats, smpw = _torch_ops.call("feed_batch", points, labels, colors, normals,
                                       conv(weight, torch.float32), None, cw, bool(color),
                                       bool(normal))
    return xyz, labels.contiguous(), feats if (color or normal) else None, smpw


def choose_model(use_color=True, use_normal=True, use_attention=False, attention_single_layer=-1):
    """The reference's model choice with its three asserts (:291-293, :323-330) as a callable
    with model_body's signature: features -> pointnet2_sem_seg_features, use_attention ->
    pointnet2_sem_seg_attention, attention_single_layer != -1 ->
    pointnet2_sem_seg_attention_single_layer, else pointnet2_sem_seg."""
    assert use_color != use_attention, \
        "Attention not supported in combination with the usage of color features"
    assert use_normal != use_attention, \
        "Attention not supported in combination with the usage of color features"
    assert attention_single_layer == -1 or not use_attention, \
        "Either attention on all or a single layer"
    if use_normal or use_color:
        return model_body
    if use_attention:
        return pointnet2_sem_seg_attention.body
    if attention_single_layer != -1:
        return pointnet2_sem_seg_attention_single_layer.body(attention_single_layer)
    return model_body


def _mean(xs):
    """The mean of a list of 0-d device tensors as a float: one read."""
    return float(torch.stack([x.detach().to(torch.float64) for x in xs]).mean()) if xs else \
        float("nan")


def _accuracies(counts):
    """Per-batch correct / assigned (NaN for 0 / 0, as TensorFlow) of a list of counts: one
    read."""
    c = torch.stack(counts).to(torch.float64)
    return c[:, 0] / c[:, 1]


def eval_model(store, metrics, val_batches, use_color=True, use_normal=True, num_class=21,
               model=None, eval_fn=eval_step, device="cuda"):
    """eval_model (:221-285): one pass over `val_batches` (stored batches, get_data_tensors'
    input) with eval_fn, then (mean loss, mean accuracy, IoU) as floats: the means over the
    batches (:265-266) and the streaming mean IoU after the last one (:267). `metrics` is reset
    afterwards (:279). Nothing is read back before the last batch has been enqueued.
    Validation is weighted with its own sample weights; the reference passes the TRAINING
    batch's weights to the validation loss (:344), which is not copied."""
    losses, counts = [], []
    for batch in val_batches:
        xyz, labels, feats, smpw = get_data_tensors(batch, use_color, use_normal, device)
        loss, cnt = eval_fn(store, metrics, xyz, labels, smpw, num_class, features=feats,
                            model=model)
        losses.append(loss)
        counts.append(cnt)
    iou = float(metrics.iou()[0]) if losses else float("nan")
    acc = float(_accuracies(counts).mean()) if counts else float("nan")
    metrics.reset()
    return _mean(losses), acc, iou


def train(store, train_batches, val_batches=None, epochs=1000, batch_size=BATCH_SIZE,
          n_train_samples=N_TRAIN_SAMPLES, use_color=True, use_normal=True, use_attention=False,
          attention_single_layer=-1, n_epochs_to_val=4, save_dir=None, step_fn=None,
          eval_fn=eval_step, num_class=21, device="cuda", optimizer=None, seed=None,
          metrics=None, val_metrics=None):
    """The reference's training loop (:288-387) on a trainable store.

    train_batches: an iterable of stored batches (get_data_tensors' input), re-started when it
    runs out (the reference's dataset repeats); val_batches: a sequence of stored batches, walked
    once per validation. Model choice and asserts: choose_model. step_fn: called with
    train_step's arguments and model=<the chosen model>; None is train_step_with on that model.
    eval_fn: eval_step's arguments, model= included. Epoch arithmetic as the
    reference: batches_per_epoch = n_train_samples / batch_size (a float), int(epochs *
    batches_per_epoch) steps, step i belongs to epoch int((i + 1) / batches_per_epoch) + 1 and an
    epoch ends when (i + 1) % int(batches_per_epoch) == 0 (:358-377). Learning rate and batch-norm
    decay follow the optimiser's step count (:319-321). At an epoch's end the mean loss and mean
    accuracy (sums over batches_per_epoch, :209-210) and the streaming IoU are summarised and the
    train metrics reset; every n_epochs_to_val epochs eval_model runs, and when the validation
    IoU improves on the best so far (0 at the start) the store's and the optimiser's exports go
    to save_dir/best_model_epoch_%03d.npz (:273-276). Inside an epoch nothing reads the device
    back: losses and counts are kept as device tensors until the epoch's end. `seed`: step i's
    dropout seed is seed + i (None: drawn per step). `optimizer`, `metrics`, `val_metrics`: an
    AdamOptimizer and SegMetrics to go on from (default: fresh ones).

    One deviation, documented and not copied: the reference weights the validation loss with
    the training batch's sample weights (:344); here validation uses its own.
    Returns the per-epoch history: a list of dicts with epoch, step, loss, accuracy, iou,
    learning_rate, bn_decay and, on validation epochs, val_loss, val_accuracy, val_iou, saved."""
    model = choose_model(use_color, use_normal, use_attention, attention_single_layer)
    opt = optimizer if optimizer is not None else AdamOptimizer(store)
    if step_fn is None:
        def step_fn(*args, model=None, **kw):
            return train_step_with(model, *args, **kw)
    metrics = metrics if metrics is not None else SegMetrics(num_class, device)
    val_metrics = val_metrics if val_metrics is not None else SegMetrics(num_class, device)
    batches_per_epoch = n_train_samples / batch_size
    history, losses, counts, best_iou = [], [], [], 0
    it = iter(train_batches)
    for i in range(int(epochs * batches_per_epoch)):
        epoch = int((i + 1) / batches_per_epoch) + 1
        try:
            batch = next(it)
        except StopIteration:
            it = iter(train_batches)
            batch = next(it)
        xyz, labels, feats, smpw = get_data_tensors(batch, use_color, use_normal, device)
        lr = get_learning_rate(opt.t, batch_size, n_train_samples)
        bn_decay = get_bn_decay(opt.t, batch_size, n_train_samples)
        loss, cnt = step_fn(store, opt, metrics, xyz, labels, smpw, num_class, bn_decay=bn_decay,
                            learning_rate=lr, features=feats,
                            seed=None if seed is None else seed + i, model=model)
        losses.append(loss)
        counts.append(cnt)
        if (i + 1) % int(batches_per_epoch) == 0:
            entry = {"epoch": epoch, "step": i + 1,
                     "loss": float(torch.stack([x.detach().to(torch.float64)
                                                for x in losses]).sum()) / batches_per_epoch,
                     "accuracy": float(_accuracies(counts).sum()) / batches_per_epoch,
                     "iou": float(metrics.iou()[0]),
                     "learning_rate": get_learning_rate(opt.t, batch_size, n_train_samples),
                     "bn_decay": get_bn_decay(opt.t, batch_size, n_train_samples)}
            metrics.reset()
            losses, counts = [], []
            if val_batches is not None and epoch % n_epochs_to_val == 0:
                vl, va, vi = eval_model(store, val_metrics, val_batches, use_color, use_normal,
                                        num_class, model, eval_fn, device)
                entry.update(val_loss=vl, val_accuracy=va, val_iou=vi, saved=None)
                if vi > best_iou:
                    best_iou = vi
                    if save_dir is not None:
                        os.makedirs(save_dir, exist_ok=True)
                        path = os.path.join(save_dir, f"best_model_epoch_{epoch:03d}.npz")
                        np.savez(path, **store.state_dict(), **opt.state_dict())
                        entry["saved"] = path
            history.append(entry)
    return history
