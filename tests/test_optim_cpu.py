"""CPU: the optimiser, schedules and metrics of the training loop (csrc/optim.hip,
csrc/cpu_optim.cpp, train.py) without a GPU: the host twins against numpy, the argument checks
that return before any launch, the schedules' values, the operators' schemas, Meta kernels and
check texts, and the optimiser's state round trip. tests/test_gpu_optim.py runs the kernels."""
import ctypes
import importlib
import inspect
import math
import os

import numpy as np
import pytest
import torch

import optim_cases as oc

E = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


@pytest.fixture(scope="module")
def L(pn2):
    return importlib.import_module(pn2.__name__ + "._lib")


def test_constants_and_signatures(pn2, L):
    assert (L.PN2_ADAM_CHUNK, L.PN2_ADAM_SLOTS) == (oc.CHUNK, oc.SLOTS)
    assert L.PN2_METRICS_MAX_C == 64
    # the slot table and its chunk starts fit the 4096-byte argument block
    assert ctypes.sizeof(L.AdamSlot) == 40
    assert L.PN2_ADAM_SLOTS * (ctypes.sizeof(L.AdamSlot) + 4) + 4 + 5 * 4 <= 4096
    P, I, F, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    assert L.SIGNATURES["pn2_adam_step"] == (I, [P, I, F, F, F, F, P])
    assert L.SIGNATURES["pn2cpu_adam_step"] == (I, [P, I, F, F, F, F])
    assert L.SIGNATURES["pn2_seg_confusion"] == (I, [P, P, LL, I, P, P, P])
    assert L.SIGNATURES["pn2cpu_seg_confusion"] == (I, [P, P, LL, I, P, P])
    assert L.SIGNATURES["pn2_mean_iou"] == (I, [P, I, P, P, P])
    assert L.SIGNATURES["pn2cpu_mean_iou"] == (I, [P, I, P, P])
    header = open(os.path.join(ROOT, "include", "pn2hip.h")).read()
    for text in (f"#define PN2_ADAM_SLOTS {oc.SLOTS}", f"#define PN2_ADAM_CHUNK {oc.CHUNK}",
                 "#define PN2_METRICS_MAX_C 64",
                 f"#define PN2_CONFUSION_BLOCK_ROWS {L.PN2_CONFUSION_BLOCK_ROWS}"):
        assert text in header, text


# ------------------------------------------------------------------------------ Adam twin
def run_twin(lib, L, arenas, grads):
    """STEPS steps of pn2cpu_adam_step over the arenas (p, g, m, v) with fresh gradients each
    step, next to the numpy float32 (and float64) restatement slot by slot."""
    ap, ag, am, av = arenas
    n = len(ap.sizes)
    ref = {dt: [[np.asarray(a.view(i), dt).copy() for a in (ap, am, av)] for i in range(n)]
           for dt in (np.float32, np.float64)}
    tab = oc.slot_table(L.AdamSlot, [oc.host_base(a.host) for a in arenas], arenas)
    for t in range(1, oc.STEPS + 1):
        alpha = oc.alpha_of(t)
        for i in range(n):
            ag.view(i)[:] = grads[t - 1][i]
        assert lib.pn2cpu_adam_step(tab, n, alpha, oc.BETA1, oc.BETA2, oc.EPSILON) == 0
        for dt in ref:
            for i in range(n):
                p, m, v = ref[dt][i]
                ref[dt][i] = list(oc.numpy_adam(p, grads[t - 1][i], m, v, alpha, oc.BETA1,
                                                oc.BETA2, oc.EPSILON, dt))
    return ref


def make_case(sizes, seed, moderate=False, offsets=None):
    rng = np.random.default_rng(seed)
    arenas = [oc.Arena(sizes, offsets).fill(rng, nonneg=k == 3, moderate=moderate)
              for k in range(4)]
    grads = [[oc.values(rng, n, moderate=moderate) for n in sizes] for _ in range(oc.STEPS)]
    return arenas, grads


def test_adam_twin_equals_numpy_float32_bit_for_bit(pn2, L):
    sizes = list(oc.SIZES) + [0, 7]
    arenas, grads = make_case(sizes, 11)
    ref = run_twin(pn2.lib(), L, arenas, grads)[np.float32]
    ap, ag, am, av = arenas
    seen = np.concatenate([g for step in grads for g in step])
    for s in oc.SPECIAL:  # the value set reached the gradients
        assert (seen == s).any(), s
    sq = seen.astype(np.float32) * seen.astype(np.float32)
    assert ((sq > 0) & (sq < np.finfo(np.float32).tiny)).any()  # g * g: a denormal
    for i, n in enumerate(sizes):
        for a, want, what in ((ap, ref[i][0], "p"), (am, ref[i][1], "m"), (av, ref[i][2], "v")):
            got = a.view(i)
            assert np.isfinite(got).all()
            assert np.array_equal(oc.bits(got), oc.bits(want)), (what, i, n)
    for a in arenas:
        assert a.guards_intact()
    # denormal second moments are kept, not flushed
    v_all = np.concatenate([av.view(i) for i in range(len(sizes))])
    assert ((v_all > 0) & (v_all < np.finfo(np.float32).tiny)).any()


def test_adam_twin_is_adam_in_float64(pn2, L):
    """Moderate values only: the twin within the project's tolerance of the same update in
    float64, max(4 * err32, 1e-6 * (1 + max |f64|)) with err32 the numpy float32 restatement's
    own error (tests/test_gpu_head_train.py)."""
    sizes = [5, oc.CHUNK + 1, 300]
    arenas, grads = make_case(sizes, 12, moderate=True)
    ref = run_twin(pn2.lib(), L, arenas, grads)
    for i in range(len(sizes)):
        for k, a in enumerate((arenas[0], arenas[2], arenas[3])):
            r64, r32 = ref[np.float64][i][k], ref[np.float32][i][k].astype(np.float64)
            err = np.abs(a.view(i).astype(np.float64) - r64).max()
            tol = max(4 * np.abs(r32 - r64).max(), 1e-6 * (1 + np.abs(r64).max()))
            assert err <= tol, (i, k, err, tol)


def test_adam_first_step_moves_by_the_learning_rate(pn2, L):
    """One step from zero slots and p = 0: m' = g (1 - b1), v' = g^2 (1 - b2), alpha = lr
    sqrt(1 - b2) / (1 - b1), so p' = -lr g / (|g| + eps / sqrt(1 - b2)): -lr sign(g) up to
    eps / (|g| sqrt(1 - b2)) <= 1e-8 / (0.1 * 0.0316) = 3.2e-6 relative for |g| >= 0.1, plus a
    few fp32 roundings (6e-8 each): 1e-5 covers both."""
    rng = np.random.default_rng(3)
    n = 1000
    g = (rng.uniform(0.1, 10.0, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.float32)
    arenas = [oc.Arena([n]) for _ in range(4)]
    for a in arenas:
        a.view(0)[:] = 0
    arenas[1].view(0)[:] = g
    tab = oc.slot_table(L.AdamSlot, [oc.host_base(a.host) for a in arenas], arenas)
    assert pn2.lib().pn2cpu_adam_step(tab, 1, oc.alpha_of(1), oc.BETA1, oc.BETA2, oc.EPSILON) == 0
    step = -arenas[0].view(0).astype(np.float64)
    np.testing.assert_allclose(step, oc.LR * np.sign(g), rtol=1e-5, atol=0)


def test_adam_argument_errors_without_a_device(pn2, L):
    lib = pn2.lib()
    fake = 1 << 20
    S = L.AdamSlot
    ok = (0.001, 0.9, 0.999, 1e-8)
    one = lambda *f: (S * 1)(S(*f))  # noqa: E731
    for fn, tail in ((lib.pn2_adam_step, (None,)), (lib.pn2cpu_adam_step, ())):
        assert fn(None, 1, *ok, *tail) == E                            # null table
        assert fn(None, -1, *ok, *tail) == E
        for k in range(4):                                             # a null pointer, n > 0
            ptrs = [fake] * 4
            ptrs[k] = None
            assert fn(one(*ptrs, 8), 1, *ok, *tail) == E, k
        assert fn(one(fake, fake, fake, fake, -1), 1, *ok, *tail) == E  # n < 0
        assert fn(one(fake, fake, fake, fake, L.PN2_ADAM_MAX_N + 1), 1, *ok, *tail) == E
        empty = one(None, None, None, None, 0)
        for b in (-0.1, 1.0, 1.5, float("nan")):
            assert fn(empty, 1, 0.001, b, 0.999, 1e-8, *tail) == E, b   # beta1
            assert fn(empty, 1, 0.001, 0.9, b, 1e-8, *tail) == E, b     # beta2
        assert fn(empty, 1, 0.001, 0.9, 0.999, -1e-8, *tail) == E       # epsilon < 0
        assert fn(empty, 1, 0.001, 0.9, 0.999, float("nan"), *tail) == E
        for a in (float("inf"), -float("inf"), float("nan")):
            assert fn(empty, 1, a, 0.9, 0.999, 1e-8, *tail) == E, a     # alpha
        # nothing to do is no error and no launch
        assert fn(None, 0, *ok, *tail) == 0
        assert fn(empty, 1, *ok, *tail) == 0
        assert fn(empty, 1, 0.001, 0.0, 0.0, 0.0, *tail) == 0           # the closed ends


# ------------------------------------------------------------------------------ metrics
def test_confusion_argument_errors_without_a_device(pn2):
    lib = pn2.lib()
    fake = 1 << 20
    for fn, tail in ((lib.pn2_seg_confusion, (None,)), (lib.pn2cpu_seg_confusion, ())):
        assert fn(fake, fake, 10, 0, fake, fake, *tail) == E     # C = 0
        assert fn(fake, fake, 10, 65, fake, fake, *tail) == E    # C > PN2_METRICS_MAX_C
        assert fn(fake, fake, 10, -3, fake, fake, *tail) == E
        assert fn(fake, fake, -1, 21, fake, fake, *tail) == E    # rows < 0
        for k in range(4):
            ptrs = [fake] * 4
            ptrs[k] = None
            assert fn(ptrs[0], ptrs[1], 10, 21, ptrs[2], ptrs[3], *tail) == E, k
        assert fn(None, None, 0, 21, None, None, *tail) == 0     # no rows: no launch
    for fn, tail in ((lib.pn2_mean_iou, (None,)), (lib.pn2cpu_mean_iou, ())):
        assert fn(fake, 0, fake, None, *tail) == E
        assert fn(fake, 65, fake, None, *tail) == E
        assert fn(None, 21, fake, None, *tail) == E
        assert fn(fake, 21, None, None, *tail) == E


def twin_confusion(lib, labels, pred, C, cm=None, counts=None):
    cm = np.zeros((C, C), np.int64) if cm is None else cm
    counts = np.zeros(2, np.int64) if counts is None else counts
    assert lib.pn2cpu_seg_confusion(oc.host_base(labels), oc.host_base(pred), len(labels), C,
                                    oc.host_base(cm), oc.host_base(counts)) == 0
    return cm, counts


def twin_iou(lib, cm, per_class=True):
    C = cm.shape[0]
    iou, per = np.full(1, -1, np.float32), np.full(C, -1, np.float32)
    assert lib.pn2cpu_mean_iou(oc.host_base(cm), C, oc.host_base(iou),
                               oc.host_base(per) if per_class else None) == 0
    return iou[0], per


@pytest.mark.parametrize("C", [2, 21, 64])
def test_confusion_and_mean_iou_twins_equal_numpy(pn2, C):
    lib = pn2.lib()
    rng = np.random.default_rng(C)
    la, pa = oc.confusion_inputs(rng, 5000, C)
    lb, pb = oc.confusion_inputs(rng, 777, C)
    assert (la == 0).any() and (la >= C).any() and (la < 0).any()
    assert (pa < 0).any() and (pa >= C).any()
    cm, counts = twin_confusion(lib, la, pa, C)
    want_cm, want_counts = oc.numpy_confusion(la, pa, C)
    assert np.array_equal(cm, want_cm) and np.array_equal(counts, want_counts)
    assert cm[0].sum() == 0 and 0 < counts[0] < counts[1] < 5000
    # a second call accumulates
    twin_confusion(lib, lb, pb, C, cm, counts)
    cm2, counts2 = oc.numpy_confusion(lb, pb, C)
    assert np.array_equal(cm, want_cm + cm2) and np.array_equal(counts, want_counts + counts2)
    iou, per = twin_iou(lib, cm)
    mean64, per64 = oc.numpy_iou(cm)
    assert oc.bits(np.float32(iou)) == oc.bits(np.float32(mean64))
    assert np.array_equal(oc.bits(per), oc.bits(per64.astype(np.float32)))
    if C > 2:  # class C - 1 never occurs: den = 0, read as 0 and left out of the mean
        assert per[C - 1] == 0 and cm[C - 1].sum() == 0 and cm[:, C - 1].sum() == 0
        valid = [c for c in range(C) if cm[c].sum() + cm[:, c].sum() > 0]
        assert C - 1 not in valid and len(valid) < C
        assert abs(float(iou) - per64[valid].mean()) < 1e-6
    assert twin_iou(lib, cm, per_class=False)[0] == iou


def test_all_unannotated_batch(pn2):
    lib = pn2.lib()
    labels = np.zeros(100, np.int32)
    pred = np.arange(100, dtype=np.int32) % 21
    cm, counts = twin_confusion(lib, labels, pred, 21)
    assert not cm.any() and counts.tolist() == [0, 0]
    iou, per = twin_iou(lib, cm)
    assert iou == 0 and not per.any()
    assert math.isnan(pn2.train.SegMetrics.accuracy(torch.tensor([0, 0])))
    assert pn2.train.SegMetrics.accuracy(torch.tensor([3, 4])) == 0.75


# ------------------------------------------------------------------------------ schedules
def test_learning_rate_schedule(pn2):
    lr = pn2.train.get_learning_rate
    assert 6005 * 16 == 1201 * 80
    assert lr(0) == 1e-3 and lr(6004) == 1e-3
    assert lr(6005) == 1e-3 * 0.7 and lr(2 * 6005 - 1) == 1e-3 * 0.7
    assert lr(2 * 6005) == 1e-3 * 0.7 ** 2
    # the floor: 0.7 ** 12 = 1.38e-2 > 1e-2 > 0.7 ** 13 = 9.7e-3
    assert lr(12 * 6005) == 1e-3 * 0.7 ** 12 > 1e-5
    assert lr(13 * 6005) == 1e-5 and lr(13 * 6005 - 1) > 1e-5 and lr(10 ** 7) == 1e-5
    assert lr(10, batch_size=8, n_train_samples=1) == 1e-3 * 0.7      # 80 // 80
    assert isinstance(lr(3), float)


def test_bn_decay_schedule(pn2):
    bd = pn2.train.get_bn_decay
    assert bd(0) == 0.5 and bd(6004) == 0.5 and bd(6005) == 0.75
    assert bd(5 * 6005) == 0.984375 and bd(6 * 6005 - 1) == 0.984375
    assert bd(6 * 6005) == 0.99 and bd(50 * 6005) == 0.99             # 1 - 2^-7 > 0.99
    assert isinstance(bd(3), float)


# ------------------------------------------------------------------------------ operators
def test_schemas_and_kernels(ops):
    assert str(ops.adam_step._schemas[""]) == (
        "pn2::adam_step(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] exp_avg, "
        "Tensor(c!)[] exp_avg_sq, float alpha, float beta1, float beta2, float epsilon) -> ()")
    assert str(ops.seg_confusion._schemas[""]) == (
        "pn2::seg_confusion(Tensor labels, Tensor pred, Tensor(a!) confusion, "
        "Tensor(b!) counts) -> ()")
    assert str(ops.mean_iou._schemas[""]) == "pn2::mean_iou(Tensor confusion) -> (Tensor, Tensor)"
    for name in ("adam_step", "seg_confusion", "mean_iou"):
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU") and not has("Autograd")


def m_(*s, dtype=torch.float32):
    return torch.empty(s, device="meta", dtype=dtype)


def test_meta_kernels(ops):
    p = [m_(3, 4), m_(7)]
    assert ops.adam_step(p, [m_(3, 4), m_(7)], [m_(3, 4), m_(7)], [m_(12), m_(7)], 1e-3, 0.9,
                         0.999, 1e-8) is None
    i32, i64 = torch.int32, torch.int64
    assert ops.seg_confusion(m_(2, 50, dtype=i32), m_(2, 50, dtype=i32), m_(21, 21, dtype=i64),
                             m_(2, dtype=i64)) is None
    iou, per = ops.mean_iou(m_(21, 21, dtype=i64))
    assert iou.shape == () and per.shape == (21,) and iou.dtype == per.dtype == torch.float32


I32, I64 = torch.int32, torch.int64


@pytest.mark.parametrize("call,msg", [
    (lambda o: o.adam_step([m_(4)], [m_(4), m_(4)], [m_(4)], [m_(4)], 1e-3, 0.9, 0.999, 1e-8),
     "adam_step expects four lists of one length, got 1, 2, 1, 1"),
    (lambda o: o.adam_step([m_(4)], [m_(4)], [m_(4, dtype=torch.float64)], [m_(4)], 1e-3, 0.9,
                           0.999, 1e-8),
     "adam_step expects float32 tensors, got Double in exp_avg[0]"),
    (lambda o: o.adam_step([m_(4, 6)], [m_(6, 4).t()], [m_(4, 6)], [m_(4, 6)], 1e-3, 0.9, 0.999,
                           1e-8),
     "adam_step expects contiguous tensors: grads[0] is not"),
    (lambda o: o.adam_step([m_(4), m_(5)], [m_(4), m_(5)], [m_(4), m_(5)], [m_(4), m_(6)], 1e-3,
                           0.9, 0.999, 1e-8),
     "adam_step expects exp_avg_sq[1] with the 5 elements of params[1], got 6"),
    (lambda o: o.adam_step([m_(4)], [torch.zeros(4)], [m_(4)], [m_(4)], 1e-3, 0.9, 0.999, 1e-8),
     "adam_step expects every tensor on one device: grads[0] is on cpu, params[0] on meta"),
    (lambda o: o.seg_confusion(m_(10, dtype=I64), m_(10, dtype=I32), m_(21, 21, dtype=I64),
                               m_(2, dtype=I64)),
     "seg_confusion expects int32 labels and pred, got Long and Int"),
    (lambda o: o.seg_confusion(m_(10, dtype=I32), m_(9, dtype=I32), m_(21, 21, dtype=I64),
                               m_(2, dtype=I64)),
     "seg_confusion expects labels and pred of one shape: labels [10], pred [9]"),
    (lambda o: o.seg_confusion(m_(10, dtype=I32), m_(10, dtype=I32), m_(21, 20, dtype=I64),
                               m_(2, dtype=I64)),
     "seg_confusion expects a contiguous int64 (C, C) confusion with 0 < C <= 64, got Long "
     "[21, 20]"),
    (lambda o: o.seg_confusion(m_(10, dtype=I32), m_(10, dtype=I32), m_(65, 65, dtype=I64),
                               m_(2, dtype=I64)),
     "seg_confusion expects a contiguous int64 (C, C) confusion with 0 < C <= 64"),
    (lambda o: o.seg_confusion(m_(10, dtype=I32), m_(10, dtype=I32), m_(21, 21, dtype=I32),
                               m_(2, dtype=I64)),
     "confusion with 0 < C <= 64, got Int [21, 21]"),
    (lambda o: o.seg_confusion(m_(10, dtype=I32), m_(10, dtype=I32), m_(21, 21, dtype=I64),
                               m_(3, dtype=I64)),
     "seg_confusion expects int64 (2,) counts, got Long [3]"),
    (lambda o: o.mean_iou(m_(0, 0, dtype=I64)),
     "mean_iou expects a contiguous int64 (C, C) confusion with 0 < C <= 64, got Long [0, 0]"),
    (lambda o: o.mean_iou(m_(21, 21)), "mean_iou expects a contiguous int64 (C, C) confusion"),
])
def test_check_texts(ops, call, msg):
    with pytest.raises(ValueError) as e:
        call(ops)
    assert msg in str(e.value)


def test_no_cpu_kernel(ops):
    z = torch.zeros(4)
    with pytest.raises(NotImplementedError):
        ops.adam_step([z], [z.clone()], [z.clone()], [z.clone()], 1e-3, 0.9, 0.999, 1e-8)
    with pytest.raises(NotImplementedError):
        ops.mean_iou(torch.zeros(21, 21, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        ops.seg_confusion(torch.zeros(4, dtype=I32), torch.zeros(4, dtype=I32),
                          torch.zeros(21, 21, dtype=I64), torch.zeros(2, dtype=I64))


def test_exports(pn2):
    import pn2hip
    for name in ("train", "pointnet2_sem_seg_features", "AdamOptimizer", "SegMetrics",
                 "get_learning_rate", "get_bn_decay", "train_step"):
        assert name in pn2.__all__ and name in pn2hip.__all__, name
        assert getattr(pn2hip, name) is getattr(pn2, name)
    assert pn2hip.train is pn2.train
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(pn2.pointnet2_sem_seg_features.get_model) == [
        "point_cloud", "features", "is_training", "num_class", "bn_decay", "params"]
    assert sig(pn2.pointnet2_sem_seg.get_model) == [
        "point_cloud", "is_training", "num_class", "bn_decay", "params"]
    assert sig(pn2.train.train_step) == [
        "store", "opt", "metrics", "point_cloud", "labels", "smpw", "num_class", "bn_decay",
        "learning_rate", "features", "seed"]
    assert sig(pn2.train.AdamOptimizer.__init__)[1:] == [
        "params", "learning_rate", "beta1", "beta2", "epsilon"]
    assert pn2.pointnet2_sem_seg_features.get_loss is pn2.pointnet2_sem_seg.get_loss


# ------------------------------------------------------------------------------ state
def test_optimizer_state_round_trip(pn2):
    tu = pn2.tf_util
    store = tu.ParamStore(seed=3).trainable("cpu")
    store.conv("layer1/conv0", 3, 4)
    opt = pn2.train.AdamOptimizer(store, learning_rate=2e-3)
    names = [k for k, v in store.items() if v.requires_grad]
    assert sorted(names) == ["layer1/conv0/biases", "layer1/conv0/bn/beta",
                             "layer1/conv0/bn/gamma", "layer1/conv0/weights"]
    fresh = opt.state_dict()
    assert sorted(fresh) == sorted([f"{n}/Adam" for n in names] + [f"{n}/Adam_1" for n in names]
                                   + ["beta1_power", "beta2_power", "global_step"])
    assert fresh["global_step"] == 0 and fresh["beta1_power"] == 1 and fresh["beta2_power"] == 1
    assert all(not fresh[f"{n}/Adam"].any() and fresh[f"{n}/Adam"].dtype == np.float32
               and fresh[f"{n}/Adam"].shape == tuple(store[n].shape) for n in names)
    # a hand-made state, with slots of a variable the model has not created yet
    rng = np.random.default_rng(0)
    state = {"global_step": np.int64(7)}
    for n in names:
        state[f"{n}/Adam"] = rng.normal(size=tuple(store[n].shape)).astype(np.float32)
        state[f"{n}/Adam_1"] = rng.uniform(size=tuple(store[n].shape)).astype(np.float32)
    state["fc2/weights/Adam"] = np.full((1, 1, 4, 2), 0.25, np.float32)
    state["fc2/weights/Adam_1"] = np.full((1, 1, 4, 2), 0.5, np.float32)
    opt.load_state_dict(state)
    assert opt.t == 7
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    assert opt.alpha() == float(np.float32(2e-3 * math.sqrt(1 - b2 ** 7) / (1 - b1 ** 7)))
    assert opt.alpha(1e-4) == float(np.float32(1e-4 * math.sqrt(1 - b2 ** 7) / (1 - b1 ** 7)))
    back = opt.state_dict()
    assert back["global_step"] == 7 and back["global_step"].dtype == np.int64
    assert back["beta1_power"] == np.float32(b1 ** 7) and back["beta2_power"] == np.float32(b2 ** 7)
    for k, v in state.items():
        assert np.array_equal(back[k], v), k
    assert sorted(back) == sorted(list(state) + ["beta1_power", "beta2_power"])
    # the waiting slots go to the variable once it exists
    store.conv("fc2", 4, 2, bn=False)
    m, v = opt._slot("fc2/weights", store["fc2/weights"])
    assert m.shape == (1, 1, 4, 2) and float(m.min()) == 0.25 and float(v.max()) == 0.5
    assert not opt._slot("fc2/biases", store["fc2/biases"])[0].any()
    with pytest.raises(KeyError):
        opt.load_state_dict({"global_step": 1, "a/Adam": np.zeros(1, np.float32)})
    # a list of leaves: slots named by position
    leaves = [torch.zeros(3, requires_grad=True), torch.zeros(2, 2, requires_grad=True)]
    lst = pn2.train.AdamOptimizer(leaves)
    assert sorted(lst.state_dict()) == ["0/Adam", "0/Adam_1", "1/Adam", "1/Adam_1", "beta1_power",
                                        "beta2_power", "global_step"]
    leaves[0].grad = torch.ones(3)
    lst.zero_grad()
    assert leaves[0].grad is None
    with pytest.raises(ValueError):
        pn2.train.AdamOptimizer(leaves, beta1=1.0)
