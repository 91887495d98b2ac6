"""CPU: the training-mode segmentation head (csrc/head_train.hip, csrc/cpu_dropout.cpp;
torch.ops.pn2.dropout / softmax_xent / softmax_xent_grad; tf_util.dropout,
tf_util.sparse_softmax_cross_entropy, pointnet2_sem_seg). The Philox restatement the tests use
reproduces the Random123 known answers, the host twin pn2cpu_dropout equals it bit for bit, and
the GPU entry points reject bad arguments before any launch. No kernel runs here;
tests/test_gpu_head_train.py runs them on the MI355X."""
import ctypes
import os

import numpy as np
import pytest
import torch

from head_train_ref import dropout_ref, philox4x32_10

E = -22
BLOCK = 128  # PN2_XENT_BLOCK_ROWS (include/pn2hip.h)


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


# Random123's kat_vectors for philox4x32-10: counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KAT)
def test_philox_known_answers(counter, key, out):
    got = philox4x32_10(np.array([counter], np.uint64), np.array(key, np.uint64))[0]
    assert [int(v) for v in got] == list(out)


@pytest.mark.parametrize("seed", [1234, (7 << 32) + 99])
@pytest.mark.parametrize("keep", [0.5, 0.7, 1.0])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_cpu_dropout_equals_the_restatement(pn2, n, keep, seed):
    lib = pn2.lib()
    x = np.random.default_rng(n).uniform(-2, 2, n).astype(np.float32)
    x[x == 0] = 1.0
    out = np.full(n, np.nan, np.float32)
    assert lib.pn2cpu_dropout(x.ctypes.data, n, keep, seed, out.ctypes.data) == 0
    ref = dropout_ref(x, keep, seed)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    if keep == 1.0:
        assert np.array_equal(out.view(np.uint32), x.view(np.uint32))  # a copy
    # in place
    y = x.copy()
    assert lib.pn2cpu_dropout(y.ctypes.data, n, keep, seed, y.ctypes.data) == 0
    assert np.array_equal(y.view(np.uint32), ref.view(np.uint32))


def test_cpu_dropout_depends_on_the_whole_seed(pn2):
    """The high word of the seed is the second key word: it changes the mask."""
    x = np.ones(4096, np.float32)
    a, b = dropout_ref(x, 0.5, 5), dropout_ref(x, 0.5, 5 + (1 << 32))
    assert (a != b).any()
    out = np.empty_like(x)
    assert pn2.lib().pn2cpu_dropout(x.ctypes.data, x.size, 0.5, 5 + (1 << 32), out.ctypes.data) == 0
    assert np.array_equal(out, b)


def test_dropout_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20  # never dereferenced by the checks
    for fn, tail in ((lib.pn2_dropout, (None,)), (lib.pn2cpu_dropout, ())):
        for keep in (0.0, -0.5, 1.5, float("nan"), float("inf")):
            assert fn(fake, 100, keep, 1, fake, *tail) == E, keep
        assert fn(fake, -1, 0.5, 1, fake, *tail) == E
        assert fn(None, 100, 0.5, 1, fake, *tail) == E
        assert fn(fake, 100, 0.5, 1, None, *tail) == E
        assert fn(None, 0, 0.5, 1, None, *tail) == 0      # nothing to do: no launch
        assert fn(None, 0, 2.0, 1, None, *tail) == E      # the attribute is still checked


def test_xent_workspace_size(pn2):
    lib = pn2.lib()
    # one fp32 partial and one int32 count per block of PN2_XENT_BLOCK_ROWS rows
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "pn2hip.h")).read()
    assert f"#define PN2_XENT_BLOCK_ROWS {BLOCK}\n" in header
    assert lib.pn2_softmax_xent_workspace_size(0) == 0
    assert lib.pn2_softmax_xent_workspace_size(-3) == 0
    assert lib.pn2_softmax_xent_workspace_size(1) == 8
    assert lib.pn2_softmax_xent_workspace_size(BLOCK - 1) == 8
    assert lib.pn2_softmax_xent_workspace_size(BLOCK) == 8
    assert lib.pn2_softmax_xent_workspace_size(BLOCK + 1) == 16
    assert lib.pn2_softmax_xent_workspace_size(131072) == 131072 // BLOCK * 8


def test_xent_entry_points_check_arguments_without_launching(pn2):
    lib = pn2.lib()
    fake = 1 << 20
    ws = lib.pn2_softmax_xent_workspace_size(300)
    names = ("logits", "labels", "weights", "rows", "C", "lse", "pred", "loss", "num_present",
             "ws", "ws_bytes", "stream")
    ok = (fake, fake, fake, 300, 21, fake, fake, fake, fake, fake, ws, None)

    def fwd(**kw):
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.pn2_softmax_xent_fwd(*[args[n] for n in names])

    for name in ("logits", "labels", "lse", "loss", "num_present", "ws"):
        assert fwd(**{name: None}) == E, name
    assert fwd(rows=0) == E and fwd(rows=-1) == E and fwd(rows=1 << 31) == E
    assert fwd(C=0) == E and fwd(C=-2) == E and fwd(C=65536) == E
    assert fwd(ws_bytes=ws - 1) == E
    assert fwd(rows=1 << 31, ws_bytes=1 << 40) == E

    bnames = ("grad_loss", "logits", "labels", "weights", "lse", "num_present", "rows", "C",
              "grad_logits", "stream")
    bok = (fake, fake, fake, fake, fake, fake, 300, 21, fake, None)

    def bwd(**kw):
        args = dict(zip(bnames, bok))
        args.update(kw)
        return lib.pn2_softmax_xent_bwd(*[args[n] for n in bnames])

    for name in ("grad_loss", "logits", "labels", "lse", "num_present", "grad_logits"):
        assert bwd(**{name: None}) == E, name
    assert bwd(rows=0) == E and bwd(rows=1 << 31) == E
    assert bwd(C=0) == E and bwd(C=65536) == E


def test_schemas(ops):
    assert str(ops.dropout._schemas[""]) == "pn2::dropout(Tensor x, float keep_prob, int seed) -> Tensor"
    assert str(ops.softmax_xent._schemas[""]) == (
        "pn2::softmax_xent(Tensor logits, Tensor labels, Tensor? weights) -> "
        "(Tensor loss, Tensor lse, Tensor pred, Tensor num_present)")
    assert str(ops.softmax_xent_grad._schemas[""]) == (
        "pn2::softmax_xent_grad(Tensor grad_loss, Tensor logits, Tensor labels, Tensor? weights, "
        "Tensor lse, Tensor num_present) -> Tensor")
    for name in ("dropout", "softmax_xent", "softmax_xent_grad"):
        assert name in ops.NAMES
        has = lambda key: torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key)  # noqa: E731
        assert has("CUDA") and has("Meta") and not has("CPU")
    for name in ("dropout", "softmax_xent"):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", "Autograd")


def test_meta_shapes_and_autograd(ops):
    m = lambda *s, **k: torch.empty(s, device="meta", **k)  # noqa: E731
    x = m(2, 10, 128, requires_grad=True)
    y = ops.dropout(x, 0.5, 7)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.requires_grad
    y.sum().backward()
    assert x.grad.shape == x.shape
    z = m(2, 10, 21, requires_grad=True)
    lab, w = m(2, 10, dtype=torch.int32), m(2, 10)
    loss, lse, pred, n = ops.softmax_xent(z, lab, w)
    assert loss.shape == n.shape == () and lse.shape == pred.shape == (2, 10)
    assert lse.dtype == torch.float32 and pred.dtype == n.dtype == torch.int32
    assert loss.requires_grad and not (lse.requires_grad or pred.requires_grad or n.requires_grad)
    loss.backward()
    assert z.grad.shape == z.shape
    g = ops.softmax_xent_grad(m(), z.detach(), lab, None, lse, n)
    assert g.shape == z.shape


@pytest.mark.parametrize("call", [
    lambda o, m: o.dropout(m(10), 0.0, 1),                                      # keep_prob
    lambda o, m: o.dropout(m(10), 1.5, 1),
    lambda o, m: o.dropout(m(10, dtype=torch.float64), 0.5, 1),                 # dtype
    lambda o, m: o.softmax_xent(m(10, 21), m(10, dtype=torch.int64), None),     # labels int64
    lambda o, m: o.softmax_xent(m(10, 21), m(9, dtype=torch.int32), None),      # rows
    lambda o, m: o.softmax_xent(m(2, 5, 21), m(10, dtype=torch.int32), None),   # leading dims
    lambda o, m: o.softmax_xent(m(10, 21), m(10, dtype=torch.int32), m(9)),     # weights
    lambda o, m: o.softmax_xent(m(10, 21), m(10, dtype=torch.int32), m(10, 1)),
    lambda o, m: o.softmax_xent(m(10, 0), m(10, dtype=torch.int32), None),      # C = 0
    lambda o, m: o.softmax_xent(m(), m(dtype=torch.int32), None),               # no class axis
    lambda o, m: o.softmax_xent(m(10, 21, dtype=torch.float64), m(10, dtype=torch.int32), None),
    lambda o, m: o.softmax_xent_grad(m(2), m(10, 21), m(10, dtype=torch.int32), None, m(10),
                                     m(dtype=torch.int32)),                     # grad_loss
    lambda o, m: o.softmax_xent_grad(m(), m(10, 21), m(10, dtype=torch.int32), None, m(9),
                                     m(dtype=torch.int32)),                     # lse
    lambda o, m: o.softmax_xent_grad(m(), m(10, 21), m(10, dtype=torch.int32), None, m(10),
                                     m()),                                      # num_present dtype
])
def test_shape_errors(ops, call):
    m = lambda *s, **k: torch.empty(s, device="meta", **k)  # noqa: E731
    with pytest.raises(ValueError):
        call(ops, m)


def test_no_cpu_kernel(ops):
    with pytest.raises(NotImplementedError):
        ops.dropout(torch.zeros(10), 0.5, 1)
    lab = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(NotImplementedError):
        ops.softmax_xent(torch.zeros(10, 21), lab, None)
    with pytest.raises(NotImplementedError):
        ops.softmax_xent_grad(torch.ones(()), torch.zeros(10, 21), lab, None, torch.zeros(10),
                              torch.zeros((), dtype=torch.int32))


def test_tf_util_dropout_without_training_and_noise_shape(pn2):
    tu = pn2.tf_util
    x = torch.zeros(2, 8, 128)
    assert tu.dropout(x, False, "dp1") is x
    assert tu.dropout(x, False, "dp1", keep_prob=0.3, seed=5) is x
    with pytest.raises(NotImplementedError):
        tu.dropout(x, True, "dp1", noise_shape=[2, 1, 128])
    with pytest.raises(NotImplementedError):
        tu.dropout(x, False, "dp1", noise_shape=[2, 1, 128])


def test_tf_util_dropout_draws_its_seed_from_the_cpu_generator(pn2, monkeypatch):
    """seed=None: one draw from torch's default CPU generator, so torch.manual_seed fixes it."""
    tu = pn2.tf_util
    seen = []
    monkeypatch.setattr(tu._torch_ops, "call", lambda name, x, keep, seed: seen.append(
        (name, keep, seed)) or x)
    monkeypatch.setattr(tu, "device_tensor", lambda t, *_: t)
    x = torch.zeros(4)
    torch.manual_seed(11)
    tu.dropout(x, True, "dp1")
    tu.dropout(x, True, "dp1")
    torch.manual_seed(11)
    tu.dropout(x, True, "dp1", keep_prob=0.7)
    tu.dropout(x, True, "dp1", seed=42)
    assert [s[0] for s in seen] == ["dropout"] * 4
    assert seen[0][2] != seen[1][2] and seen[0][2] == seen[2][2] and seen[3][2] == 42
    assert all(isinstance(s[2], int) and 0 <= s[2] < 2 ** 62 for s in seen)
    assert seen[0][1] == 0.5 and seen[2][1] == 0.7


def test_module_is_exported(pn2):
    assert "pointnet2_sem_seg" in pn2.__all__
    mod = pn2.pointnet2_sem_seg
    assert callable(mod.get_model) and callable(mod.get_loss)
    import inspect
    assert list(inspect.signature(mod.get_model).parameters) == [
        "point_cloud", "is_training", "num_class", "bn_decay", "params"]
    assert list(inspect.signature(mod.get_loss).parameters) == ["pred", "label", "smpw"]
    assert list(inspect.signature(pn2.tf_util.dropout).parameters) == [
        "inputs", "is_training", "scope", "keep_prob", "noise_shape", "seed"]
    assert [s[0] for s in mod.SA_LAYERS] == ["layer1", "layer2", "layer3", "layer4"]
    assert [s[0] for s in mod.FP_LAYERS] == ["fa_layer1", "fa_layer2", "fa_layer3", "fa_layer4"]


def test_ctypes_seed_is_64_bit(pn2):
    _lib = __import__("importlib").import_module(pn2.__name__ + "._lib")
    assert _lib.SIGNATURES["pn2_dropout"][1][3] is ctypes.c_uint64
    assert _lib.SIGNATURES["pn2cpu_dropout"][1][3] is ctypes.c_uint64
