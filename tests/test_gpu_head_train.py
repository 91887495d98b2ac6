"""GPU: the training-mode segmentation head (csrc/head_train.hip) through torch.ops.pn2, the C
ABI and the public tf_util / pointnet2_sem_seg interfaces.

Dropout is compared bit for bit with the host twin pn2cpu_dropout (which
tests/test_head_train_cpu.py ties to a numpy restatement of Philox4x32-10 and to Random123's
known answers). The loss is compared with the float64 formula lse - z[label] under TF's
SUM_BY_NONZERO_WEIGHTS reduction and its autograd (head_train_ref.xent_ref). Tolerance (the
project's, tests/support.py):

    max |gpu - f64|  <=  max(4 * max |fp32 - f64|,  1e-6 * (1 + max |f64|))

where fp32 is the same reference function evaluated in float32 on the CPU.
"""
import functools
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from head_train_ref import xent_ref
from support import assert_close, gpu_marks, raw_bits

pytestmark = gpu_marks

BLOCK = 128  # PN2_XENT_BLOCK_ROWS (include/pn2hip.h)
XENT_C = [1, 2, 21, 50, 64, 65, 200]   # both layouts, the even-C padding, the boundary
XENT_ROWS = [1, 2, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 1, 4099]
DROP_N = [1, 5, 4 * 256 * 3 + 2, 1000 * 128]
DROP_KEEP = [0.5, 0.7]
SEED = 1234


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


# ------------------------------------------------------------------------------ dropout
def cpu_dropout(pkg, x_np, keep, seed):
    out = np.empty_like(x_np)
    assert pkg.lib().pn2cpu_dropout(x_np.ctypes.data, x_np.size, keep, seed, out.ctypes.data) == 0
    return out


def drop_input(n):
    x = np.random.default_rng(n).uniform(-3, 3, n).astype(np.float32)
    x[x == 0] = 1.0  # no zeros: the output's support is the mask
    return x


@pytest.mark.parametrize("keep", DROP_KEEP)
@pytest.mark.parametrize("n", DROP_N)
def test_dropout_equals_the_host_twin(env, n, keep):
    pkg, ops, torch, dev = env
    x_np = drop_input(n)
    ref = cpu_dropout(pkg, x_np, keep, SEED)
    x = torch.from_numpy(x_np).to(dev)
    assert x.data_ptr() % 16 == 0
    out = ops.dropout(x, keep, SEED)
    assert np.array_equal(raw_bits(out), ref.view(np.uint32))
    # a view whose storage starts one float into an allocation: the scalar path
    base = torch.empty(n + 1, device=dev)
    view = base[1:]
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    assert np.array_equal(raw_bits(ops.dropout(view, keep, SEED)), ref.view(np.uint32))
    # in place through the C ABI, aligned and not
    for t in (x.clone(), view):
        rc = pkg.lib().pn2_dropout(t.data_ptr(), n, keep, SEED, t.data_ptr(),
                                   torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(raw_bits(t), ref.view(np.uint32))


def test_dropout_keep_prob_one_copies_and_empty(env):
    pkg, ops, torch, dev = env
    x = torch.from_numpy(drop_input(1027)).to(dev)
    assert torch.equal(ops.dropout(x, 1.0, SEED), x)
    assert ops.dropout(x[:0], 0.5, SEED).shape == (0,)
    assert ops.dropout(x.reshape(13, 79)[:, :0], 0.5, SEED).shape == (13, 0)


def test_dropout_backward_is_the_op_on_the_gradient(env):
    pkg, ops, torch, dev = env
    n, keep = 4 * 256 * 3 + 2, 0.7
    x = torch.from_numpy(drop_input(n)).to(dev).reshape(2, -1).requires_grad_(True)
    go = torch.from_numpy(drop_input(n + 1)[:n]).to(dev).reshape(2, -1)
    out = ops.dropout(x, keep, SEED)
    out.backward(go)
    assert np.array_equal(raw_bits(x.grad), raw_bits(ops.dropout(go, keep, SEED)))
    # supported exactly where the output is
    assert torch.equal(x.grad != 0, out != 0)
    assert np.array_equal(raw_bits(x.grad), cpu_dropout(pkg, go.cpu().numpy().reshape(-1), keep,
                                                    SEED).view(np.uint32).reshape(2, -1))


def test_dropout_is_a_function_of_the_seed(env):
    pkg, ops, torch, dev = env
    x = torch.from_numpy(drop_input(128000)).to(dev)
    a, b = ops.dropout(x, 0.5, SEED), ops.dropout(x, 0.5, SEED)
    assert np.array_equal(raw_bits(a), raw_bits(b))
    c = ops.dropout(x, 0.5, SEED + 1)
    d = ops.dropout(x, 0.5, SEED + (1 << 32))  # the high word is part of the key
    assert not torch.equal(a != 0, c != 0) and not torch.equal(a != 0, d != 0)


@pytest.mark.parametrize("keep", DROP_KEEP)
def test_dropout_keeps_the_expected_share(env, keep):
    """Within 5 sigma of keep_prob over 128,000 elements, sigma = sqrt(p (1 - p) / n) (the
    convention gives 0.5021 at 0.5 and 0.7024 at 0.7 for this seed: under 2 sigma)."""
    pkg, ops, torch, dev = env
    n = 128000
    x = torch.from_numpy(drop_input(n)).to(dev)
    share = float((ops.dropout(x, keep, SEED) != 0).sum()) / n
    sigma = np.sqrt(keep * (1 - keep) / n)
    print(f"keep {keep}: share {share:.4f}, {abs(share - keep) / sigma:.2f} sigma")
    assert abs(share - keep) <= 5 * sigma


def test_tf_util_dropout_on_the_device(env):
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    x = torch.from_numpy(drop_input(2 * 40 * 128)).to(dev).reshape(2, 40, 128)
    assert tu.dropout(x, False, "dp1") is x
    a = tu.dropout(x, True, "dp1", keep_prob=0.5, seed=SEED)
    assert np.array_equal(raw_bits(a), raw_bits(ops.dropout(x, 0.5, SEED)))
    torch.manual_seed(3)
    b = tu.dropout(x, True, "dp1")
    torch.manual_seed(3)
    c = tu.dropout(x, True, "dp1")
    d = tu.dropout(x, True, "dp1")
    assert torch.equal(b, c) and not torch.equal(c != 0, d != 0)


# ------------------------------------------------------------------------------ the loss
def xent_inputs(torch, rows, C, seed=None):
    g = torch.Generator().manual_seed(rows * 1000 + C if seed is None else seed)
    z = (torch.rand(rows, C, generator=g, dtype=torch.float64) * 8 - 4).float()
    # every class occurs as a label (as far as the rows reach), in a shuffled order
    labels = (torch.arange(rows) % C)[torch.randperm(rows, generator=g)].to(torch.int32)
    # ScanNet's smpw: about 30 % exactly 0 (unannotated), the rest in [0.5, 5]
    w = (torch.rand(rows, generator=g, dtype=torch.float64) * 4.5 + 0.5).float()
    w[torch.rand(rows, generator=g) < 0.3] = 0.0
    w[0] = 1.25  # at least one present row
    if C > 1:    # no ties: the argmax is unique
        top = z.topk(2, dim=-1).values
        assert (top[:, 0] > top[:, 1]).all()
    return z, labels, w


@functools.lru_cache(maxsize=None)
def run_xent(rows, C):
    """Forward + backward (through autograd) of one case on the GPU and its references."""
    import torch
    import pn2hip
    ops, dev = pn2hip.ops, torch.device("cuda:0")
    z, labels, w = xent_inputs(torch, rows, C)
    zd = z.to(dev).requires_grad_(True)
    loss, lse, pred, n = ops.softmax_xent(zd, labels.to(dev), w.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    ref = {}
    for dt in (torch.float64, torch.float32):
        l, s, leaf = xent_ref(torch, z, labels, w, dt)
        l.backward()
        ref[dt] = (l.detach(), s.detach(), leaf.grad)
    return dict(z=z, labels=labels, w=w, loss=loss.detach().cpu(), lse=lse.cpu(), pred=pred.cpu(),
                n=n.cpu(), grad=zd.grad.cpu(), ref=ref)


@pytest.mark.parametrize("rows", XENT_ROWS)
@pytest.mark.parametrize("C", XENT_C)
def test_xent_forward_and_backward(env, C, rows):
    pkg, ops, torch, dev = env
    r = run_xent(rows, C)
    r64, r32 = r["ref"][torch.float64], r["ref"][torch.float32]
    assert r["loss"].shape == () and r["n"].shape == () and r["n"].dtype == torch.int32
    assert int(r["n"]) == int((r["w"] != 0).sum())
    assert r["pred"].dtype == torch.int32
    assert torch.equal(r["pred"].long(), r["z"].argmax(dim=-1))
    assert_close(r["loss"], r64[0], r32[0], f"loss rows={rows} C={C}")
    assert_close(r["lse"], r64[1], r32[1], f"lse rows={rows} C={C}")
    assert_close(r["grad"], r64[2], r32[2], f"grad_logits rows={rows} C={C}")
    assert set(r["labels"].tolist()) == set(range(min(rows, C)))


@pytest.mark.parametrize("C", [21, 200])
def test_xent_two_runs_give_equal_bits(env, C):
    pkg, ops, torch, dev = env
    z, labels, w = (t.to(dev) for t in xent_inputs(torch, 4099, C))
    runs = []
    for _ in range(2):
        loss, lse, pred, n = ops.softmax_xent(z, labels, w)
        g = ops.softmax_xent_grad(torch.full((), 0.75, device=dev), z, labels, w, lse, n)
        runs.append((loss, lse, pred, n, g))
    for a, b in zip(*runs):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint32),
                                                     b.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("C", [21, 64, 200])
def test_xent_unaligned_logits(env, C):
    """Logits that start one float into an allocation: the scalar load / store paths give the
    bits of the aligned ones."""
    pkg, ops, torch, dev = env
    rows = BLOCK + 3
    z, labels, w = (t.to(dev) for t in xent_inputs(torch, rows, C))
    base = torch.empty(rows * C + 1, device=dev)
    view = base[1:].view(rows, C)
    view.copy_(z)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    a = ops.softmax_xent(z, labels, w)
    b = ops.softmax_xent(view, labels, w)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    one = torch.ones((), device=dev)
    assert torch.equal(ops.softmax_xent_grad(one, z, labels, w, a[1], a[3]),
                       ops.softmax_xent_grad(one, view, labels, w, b[1], b[3]))


@pytest.mark.parametrize("C", [21, 200])
def test_xent_pred_takes_the_lowest_index_on_ties(env, C):
    pkg, ops, torch, dev = env
    z, labels, w = xent_inputs(torch, 70, C)
    z[3] = 0.5          # a row of equal logits
    z[4, :] = -1.0
    z[4, [C - 1, 7, 11]] = 2.0   # the maximum three times
    z[5, :] = -0.0
    z[5, 9] = 0.0       # -0 == +0: still the first
    loss, lse, pred, n = ops.softmax_xent(z.to(dev), labels.to(dev), w.to(dev))
    assert torch.equal(pred.cpu().long(), torch.from_numpy(np.argmax(z.numpy(), axis=-1)))
    assert int(pred[3]) == 0 and int(pred[4]) == 7 and int(pred[5]) == 0
    # a row of equal logits: lse - z = log C
    ref = torch.full((), np.log(C), dtype=torch.float64)
    assert_close((lse[3] - 0.5).cpu(), ref, ref.float(), f"log C, C={C}")


@pytest.mark.parametrize("C", [21, 200])
def test_xent_all_weights_zero(env, C):
    pkg, ops, torch, dev = env
    z, labels, _ = xent_inputs(torch, 2 * BLOCK + 1, C)
    zd = z.to(dev).requires_grad_(True)
    loss, lse, pred, n = ops.softmax_xent(zd, labels.to(dev), torch.zeros(len(labels), device=dev))
    loss.backward()
    assert float(loss.detach()) == 0.0 and int(n) == 0
    assert (zd.grad == 0).all() and not torch.signbit(zd.grad).any()


@pytest.mark.parametrize("C", [21, 200])
def test_xent_no_weights_and_scalar_weights(env, C):
    pkg, ops, torch, dev = env
    tu = pkg.tf_util
    z, labels, _ = xent_inputs(torch, 300, C)
    zd, ld = z.to(dev), labels.to(dev)
    none = ops.softmax_xent(zd, ld, None)
    ones = ops.softmax_xent(zd, ld, torch.ones(300, device=dev))
    for a, b in zip(none, ones):
        assert torch.equal(a, b)
    assert int(none[3]) == 300
    g_none = ops.softmax_xent_grad(torch.ones((), device=dev), zd, ld, None, none[1], none[3])
    g_ones = ops.softmax_xent_grad(torch.ones((), device=dev), zd, ld, torch.ones(300, device=dev),
                                   ones[1], ones[3])
    assert torch.equal(g_none, g_ones)
    # the public function: a scalar scales the mean, 0 gives 0, labels may be int64
    assert torch.equal(tu.sparse_softmax_cross_entropy(ld, zd), none[0])
    assert torch.equal(tu.sparse_softmax_cross_entropy(ld.long(), zd, weights=2.5), none[0] * 2.5)
    assert float(tu.sparse_softmax_cross_entropy(ld, zd, weights=0.0)) == 0.0
    r64 = xent_ref(torch, z, labels, None, torch.float64)[0].detach()
    r32 = xent_ref(torch, z, labels, None, torch.float32)[0].detach()
    assert_close(none[0].cpu(), r64, r32, f"unweighted loss C={C}")
    zr = zd.clone().requires_grad_(True)
    tu.sparse_softmax_cross_entropy(ld, zr, weights=2.5).backward()
    assert_close(zr.grad.cpu(), 2.5 * g_none.double().cpu(), 2.5 * g_none.cpu(), "scalar-weight grad")


@pytest.mark.parametrize("C", [21, 200])
def test_xent_large_logits_stay_finite(env, C):
    """Logits of +-80: exp overflows fp32 without the max subtraction."""
    pkg, ops, torch, dev = env
    z, labels, w = xent_inputs(torch, 150, C)
    z = torch.where(z > 0, torch.full_like(z, 80.0), torch.full_like(z, -80.0)) + z * 0.01
    zd = z.to(dev).requires_grad_(True)
    loss, lse, pred, n = ops.softmax_xent(zd, labels.to(dev), w.to(dev))
    loss.backward()
    ref = {}
    for dt in (torch.float64, torch.float32):
        l, s, leaf = xent_ref(torch, z, labels, w, dt)
        l.backward()
        ref[dt] = (l.detach(), s.detach(), leaf.grad)
    for got, k, what in ((loss, 0, "loss"), (lse, 1, "lse"), (zd.grad, 2, "grad")):
        assert_close(got.cpu(), ref[torch.float64][k], ref[torch.float32][k], f"+-80 {what} C={C}")


@pytest.mark.parametrize("C", [5, 70])
def test_xent_label_out_of_range_gives_nan(env, C):
    """ONE row of a small tensor carries a label outside [0, C): it is never dereferenced (an
    addressing guard, not a fault), its cross-entropy is NaN and so is the loss; lse, pred and
    the gradient do not read the label's column and stay finite."""
    pkg, ops, torch, dev = env
    z, labels, _ = xent_inputs(torch, 4, C)
    labels[2] = C + 2
    zd = z.to(dev)
    loss, lse, pred, n = ops.softmax_xent(zd, labels.to(dev), None)
    assert torch.isnan(loss) and int(n) == 4
    assert torch.isfinite(lse).all()
    assert torch.equal(pred.cpu().long(), z.argmax(dim=-1))
    g = ops.softmax_xent_grad(torch.ones((), device=dev), zd, labels.to(dev), None, lse, n)
    assert torch.isfinite(g).all()


def test_xent_empty_and_leading_dims(env):
    pkg, ops, torch, dev = env
    z = torch.zeros(0, 21, device=dev, requires_grad=True)
    loss, lse, pred, n = ops.softmax_xent(z, torch.zeros(0, dtype=torch.int32, device=dev), None)
    assert float(loss.detach()) == 0.0 and int(n) == 0 and lse.shape == pred.shape == (0,)
    # (B, N, C) logits with (B, N) labels and weights: the rows flattened
    zz, labels, w = xent_inputs(torch, 2 * 150, 21)
    a = ops.softmax_xent(zz.to(dev), labels.to(dev), w.to(dev))
    b = ops.softmax_xent(zz.view(2, 150, 21).to(dev), labels.view(2, 150).to(dev),
                         w.view(2, 150).to(dev))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(2, 150), b[1]) and b[2].shape == (2, 150)


# ------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def cloud():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    xyz = torch.from_numpy(pkg.synth.batch([0, 1], 1024, "scannet")[0]).to("cuda:0")
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, 4, (2, 1024), generator=g, dtype=torch.int32).to("cuda:0")
    w = (torch.rand(2, 1024, generator=g) * 4.5 + 0.5)
    w[torch.rand(2, 1024, generator=g) < 0.3] = 0.0
    return xyz, labels, w.to("cuda:0")


def test_model_trains_every_variable(env):
    pkg, ops, torch, dev = env
    seg = pkg.pointnet2_sem_seg
    xyz, labels, smpw = cloud()
    store = pkg.tf_util.ParamStore(seed=1).trainable("cuda:0")

    def step_loss():
        torch.manual_seed(17)  # the dropout seed is drawn from the CPU generator
        net, end_points = seg.get_model(xyz, True, 4, bn_decay=0.5, params=store)
        assert net.shape == (2, 1024, 4) and end_points["feats"].shape == (2, 1024, 128)
        assert end_points["l0_xyz"] is xyz
        return seg.get_loss(net, labels, smpw), net

    loss, net = step_loss()
    # the loss is TF's reduction of the model's own logits
    r64 = xent_ref(torch, net.detach().cpu().view(-1, 4), labels.cpu().view(-1),
                   smpw.cpu().view(-1), torch.float64)[0].detach()
    r32 = xent_ref(torch, net.detach().cpu().view(-1, 4), labels.cpu().view(-1),
                   smpw.cpu().view(-1), torch.float32)[0].detach()
    assert_close(loss.cpu(), r64, r32, "get_loss")
    loss.backward()
    params = list(store.parameters())
    names = [k for k, v in store.items() if v.requires_grad]
    assert any(k.startswith("fc2/") for k in names) and any(k.startswith("fc1/") for k in names)
    for k in names:
        assert store[k].grad is not None and torch.isfinite(store[k].grad).all(), k
    for k in ("fc2/weights", "fc2/biases", "fc1/weights", "layer1/conv0/weights",
              "fa_layer4/conv_2/weights"):
        assert float(store[k].grad.abs().max()) > 0, k
    opt = torch.optim.Adam(params, lr=1e-3)
    first = float(loss.detach())
    for _ in range(5):
        opt.zero_grad()
        loss, _ = step_loss()
        loss.backward()
        opt.step()
    last = float(step_loss()[0].detach())
    print(f"get_loss: {first:.4f} -> {last:.4f} after 5 Adam steps")
    assert np.isfinite(last) and last < first


def test_model_inference_equals_the_module_calls(env):
    """is_training=False on a plain store: the logits of the same layers called one by one
    (INTEGRATION.md section 4), bit for bit."""
    pkg, ops, torch, dev = env
    pu, tu = pkg.pointnet_util, pkg.tf_util
    xyz, _, _ = cloud()
    store = tu.ParamStore(seed=2)
    net, end_points = pkg.pointnet2_sem_seg.get_model(xyz, False, 4, params=store)
    sa = pu.pointnet_sa_module
    l1_xyz, l1_p, _ = sa(xyz, None, 1024, 0.1, 32, [32, 32, 64], None, False, False, None,
                         "layer1", params=store)
    l2_xyz, l2_p, _ = sa(l1_xyz, l1_p, 256, 0.2, 32, [64, 64, 128], None, False, False, None,
                         "layer2", params=store)
    l3_xyz, l3_p, _ = sa(l2_xyz, l2_p, 64, 0.4, 32, [128, 128, 256], None, False, False, None,
                         "layer3", params=store)
    l4_xyz, l4_p, _ = sa(l3_xyz, l3_p, 16, 0.8, 32, [256, 256, 512], None, False, False, None,
                         "layer4", params=store)
    fp = pu.pointnet_fp_module
    l3_p = fp(l3_xyz, l4_xyz, l3_p, l4_p, [256, 256], False, None, "fa_layer1", params=store)
    l2_p = fp(l2_xyz, l3_xyz, l2_p, l3_p, [256, 256], False, None, "fa_layer2", params=store)
    l1_p = fp(l1_xyz, l2_xyz, l1_p, l2_p, [256, 128], False, None, "fa_layer3", params=store)
    l0_p = fp(xyz, l1_xyz, None, l1_p, [128, 128, 128], False, None, "fa_layer4", params=store)
    feats = tu.conv1d(l0_p, 128, 1, "fc1", bn=True, is_training=False, params=store)
    want = tu.conv1d(feats, 4, 1, "fc2", activation_fn=None, params=store)
    assert net.shape == (2, 1024, 4)
    assert torch.equal(end_points["feats"], feats) and torch.equal(net, want)
