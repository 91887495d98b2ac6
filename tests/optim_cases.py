"""Shared by tests/test_optim_cpu.py and tests/test_gpu_optim.py (no tests here): the Adam value
set and slot sizes, the numpy restatement of TF 1.x ApplyAdam, and a guarded buffer layout.

The contract under test, per element, in the working dtype, every operation rounded on its own:

    omb1 = 1 - beta1;  omb2 = 1 - beta2
    m' = m + (g - m) * omb1
    v' = v + (g * g - v) * omb2
    p' = p - (alpha * m') / (sqrt(v') + epsilon)
"""
import ctypes
import math

import numpy as np

from support import raw_bits as bits  # noqa: F401  (used as oc.bits)

CHUNK = 2048   # PN2_ADAM_CHUNK (the tests assert it against _lib)
SLOTS = 64     # PN2_ADAM_SLOTS
SIZES = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)
# 0; +-1e-20 (g * g underflows to a denormal or to 0); around 1e-3 and 1; +-1e18 (g * g = 1e36
# stays finite in fp32, so no infinity or NaN arises)
SPECIAL = np.array([0.0, 1e-20, -1e-20, 1e-3, -1e-3, 1.0, -1.0, 1e18, -1e18], np.float32)
GUARD = 64          # floats of SENTINEL on both sides of every buffer
SENTINEL = np.float32(-1234.5)
BETA1, BETA2, EPSILON, LR = 0.9, 0.999, 1e-8, 1e-3
STEPS = 3


def alpha_of(t, lr=LR, beta1=BETA1, beta2=BETA2):
    """AdamOptimizer.step's step size: betas rounded to fp32 first, alpha rounded to fp32 last."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return float(np.float32(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)))


def numpy_adam(p, g, m, v, alpha, beta1, beta2, epsilon, dt):
    """The four lines above in dtype dt; beta1, beta2, alpha and epsilon are first rounded to
    fp32 (they are fp32 arguments of the C ABI). Returns (p', m', v')."""
    f = lambda x: dt(np.float32(x))  # noqa: E731
    p, g, m, v = (np.asarray(a, dt) for a in (p, g, m, v))
    omb1, omb2 = dt(1) - f(beta1), dt(1) - f(beta2)
    m2 = m + (g - m) * omb1
    v2 = v + (g * g - v) * omb2
    p2 = p - (f(alpha) * m2) / (np.sqrt(v2) + f(epsilon))
    assert p2.dtype == m2.dtype == v2.dtype == dt
    return p2, m2, v2


def values(rng, n, nonneg=False, moderate=False):
    """n float32 values: the SPECIAL set (unless moderate) mixed with magnitudes around 1e-3 and
    around 1, either sign (or none below zero)."""
    mag = np.where(rng.random(n) < 0.5, 1e-3, 1.0) * rng.uniform(0.5, 2.0, n)
    x = (mag * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    if not moderate:
        pick = rng.random(n) < 0.4
        x[pick] = SPECIAL[rng.integers(0, len(SPECIAL), int(pick.sum()))]
        x[: min(n, len(SPECIAL))] = SPECIAL[: min(n, len(SPECIAL))]  # each at least once
        rng.shuffle(x)
    return np.abs(x) if nonneg else x


class Arena:
    """One float32 host array holding every slot's buffer of one kind (p, g, m or v), each with
    GUARD floats of SENTINEL on both sides. starts[i] is slot i's first element: a multiple of 4
    floats past the arena's base, plus offsets[i] (1 moves the slot off the 16-byte boundary)."""

    def __init__(self, sizes, offsets=None):
        self.sizes = list(sizes)
        offsets = offsets if offsets is not None else [0] * len(self.sizes)
        self.starts, cur = [], 0
        for n, off in zip(self.sizes, offsets):
            self.starts.append(cur + GUARD + off)
            cur = (cur + GUARD + off + n + GUARD + 3) // 4 * 4
        self.host = np.full(max(cur, 4), SENTINEL, np.float32)

    def view(self, i, array=None):
        a = self.host if array is None else array
        return a[self.starts[i]: self.starts[i] + self.sizes[i]]

    def fill(self, rng, **kw):
        for i, n in enumerate(self.sizes):
            self.view(i)[:] = values(rng, n, **kw)
        return self

    def guards_intact(self, array=None):
        a = self.host if array is None else np.asarray(array)
        mask = np.ones(a.shape, bool)
        for s, n in zip(self.starts, self.sizes):
            mask[s: s + n] = False
        return bool((a[mask] == SENTINEL).all())


def slot_table(AdamSlot, bases, arenas):
    """ctypes array of pn2_adam_slot over the arenas (p, g, m, v) whose first elements lie at the
    byte addresses `bases`."""
    n = len(arenas[0].sizes)
    tab = (AdamSlot * max(n, 1))()
    for i in range(n):
        ptrs = [b + 4 * a.starts[i] for b, a in zip(bases, arenas)]
        tab[i] = AdamSlot(*ptrs, arenas[0].sizes[i])
    return tab


def host_base(a):
    return a.ctypes.data_as(ctypes.c_void_p).value


def cycle_sizes(nslots, zero_at=None):
    sizes = [SIZES[i % len(SIZES)] for i in range(nslots)]
    if zero_at is not None:
        sizes[zero_at] = 0
    return sizes


def confusion_inputs(rng, rows, C):
    """labels in [-2, C + 2) (0: unannotated; negative and >= C: out of range), pred in
    [-1, C + 1); class C - 1 never occurs as a label or a prediction when C > 2."""
    labels = rng.integers(-2, C + 2, rows).astype(np.int32)
    pred = rng.integers(-1, C + 1, rows).astype(np.int32)
    if C > 2:
        labels[labels == C - 1] = 1
        pred[pred == C - 1] = 1
    return labels, pred


def numpy_confusion(labels, pred, C):
    ok = (labels > 0) & (labels < C) & (pred >= 0) & (pred < C)
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (labels[ok], pred[ok]), 1)
    counts = np.array([int((labels[ok] == pred[ok]).sum()), int(ok.sum())], np.int64)
    return cm, counts


def numpy_iou(cm):
    """(mean, per_class) in float64: classes with den = 0 are left out of the mean and read 0;
    the sum runs in class order."""
    tp = np.diag(cm)
    den = cm.sum(0) + cm.sum(1) - tp  # int64, exact
    valid = den > 0
    per = np.where(valid, tp.astype(np.float64) / np.where(valid, den, 1).astype(np.float64), 0.0)
    total = 0.0
    for c in np.flatnonzero(valid):
        total += float(per[c])
    return (total / int(valid.sum()) if valid.any() else 0.0), per
