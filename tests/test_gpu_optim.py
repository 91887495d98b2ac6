"""GPU: the optimiser and metrics kernels of csrc/optim.hip against their host twins
(csrc/cpu_optim.cpp, pinned to numpy in tests/test_optim_cpu.py), bit for bit, and train.py's
AdamOptimizer, SegMetrics and train_step on trainable stores.

Every Adam buffer lies inside one device arena per kind with 64 floats of a sentinel on both
sides of every slot; the whole arena is compared with the host's, so a write outside a slot
shows as a changed guard, never as a fault."""
import functools
import importlib

import numpy as np
import pytest

import optim_cases as oc
from conftest import PKG_NAME
from support import gpu_marks

pytestmark = gpu_marks


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    import pn2hip
    L = importlib.import_module(PKG_NAME + "._lib")
    return pkg, pn2hip.ops, torch, torch.device("cuda:0"), L


# ------------------------------------------------------------------------------ Adam
def adam_case(nslots, seed):
    """Arenas (p, g, m, v) and per-step gradients. Sizes cycle through oc.SIZES; an n = 0 slot
    sits in the middle; every seventh slot has one of its four buffers one element off the
    16-byte boundary (the scalar path, between vector-path neighbours)."""
    sizes = oc.cycle_sizes(nslots, zero_at=nslots // 2 if nslots > 2 else None)
    if nslots == 1:
        sizes = [2 * oc.CHUNK + 3]
    rng = np.random.default_rng(seed)
    arenas = []
    for k in range(4):
        offsets = [1 if (i % 7 == 3 and (i // 7) % 4 == k) else 0 for i in range(nslots)]
        arenas.append(oc.Arena(sizes, offsets).fill(rng, nonneg=k == 3))
    grads = [[oc.values(rng, n) for n in sizes] for _ in range(oc.STEPS)]
    return sizes, arenas, grads


def to_device(torch, dev, arenas):
    devs = [torch.from_numpy(a.host.copy()).to(dev) for a in arenas]
    for d in devs:
        assert d.data_ptr() % 16 == 0
    return devs


def set_grads(torch, arenas, devs, step_grads):
    ag = arenas[1]
    for i, g in enumerate(step_grads):
        ag.view(i)[:] = g
    devs[1].copy_(torch.from_numpy(ag.host))


def run_host(lib, L, arenas, grads):
    tab = oc.slot_table(L.AdamSlot, [oc.host_base(a.host) for a in arenas], arenas)
    for t in range(1, oc.STEPS + 1):
        for i, g in enumerate(grads[t - 1]):
            arenas[1].view(i)[:] = g
        assert lib.pn2cpu_adam_step(tab, len(grads[0]), oc.alpha_of(t), oc.BETA1, oc.BETA2,
                                    oc.EPSILON) == 0


def run_capi(torch, lib, L, arenas, devs, grads):
    tab = oc.slot_table(L.AdamSlot, [d.data_ptr() for d in devs], arenas)
    for t in range(1, oc.STEPS + 1):
        set_grads(torch, arenas, devs, grads[t - 1])
        rc = lib.pn2_adam_step(tab, len(grads[0]), oc.alpha_of(t), oc.BETA1, oc.BETA2, oc.EPSILON,
                               L.stream_of(devs[0]))
        assert rc == 0, rc
    torch.cuda.synchronize()


def run_op(torch, ops, arenas, devs, grads):
    views = [[a.view(i, d) for i in range(len(a.sizes))] for a, d in zip(arenas, devs)]
    for t in range(1, oc.STEPS + 1):
        set_grads(torch, arenas, devs, grads[t - 1])
        ops.adam_step(views[0], views[1], views[2], views[3], oc.alpha_of(t), oc.BETA1, oc.BETA2,
                      oc.EPSILON)
    torch.cuda.synchronize()


def assert_arenas_equal(arenas, devs, what):
    for k, (a, d) in enumerate(zip(arenas, devs)):
        got = d.cpu().numpy()
        assert a.guards_intact(got), f"{what}: a guard of arena {'pgmv'[k]} changed"
        diff = np.flatnonzero(oc.bits(got) != oc.bits(a.host))
        assert diff.size == 0, (what, "pgmv"[k], diff[:8], got[diff[:8]], a.host[diff[:8]])


@pytest.mark.parametrize("nslots", [1, oc.SLOTS, oc.SLOTS + 1, 90])
def test_adam_step_equals_host_twin(env, nslots):
    pkg, ops, torch, dev, L = env
    assert (L.PN2_ADAM_CHUNK, L.PN2_ADAM_SLOTS) == (oc.CHUNK, oc.SLOTS)
    sizes, arenas, grads = adam_case(nslots, 100 + nslots)
    if nslots > 1:
        assert 0 in sizes and set(oc.SIZES) <= set(sizes)
    devs = to_device(torch, dev, arenas)
    run_capi(torch, pkg.lib(), L, arenas, devs, grads)
    run_host(pkg.lib(), L, arenas, grads)
    for a in arenas:
        assert a.guards_intact()
    assert_arenas_equal(arenas, devs, f"{nslots} slots")


def test_adam_op_equals_capi_and_repeats(env):
    pkg, ops, torch, dev, L = env
    sizes, arenas, grads = adam_case(oc.SLOTS + 5, 7)
    start = [a.host.copy() for a in arenas]
    runs = []
    for which in ("capi", "op", "op"):
        for a, s in zip(arenas, start):
            a.host[:] = s
        devs = to_device(torch, dev, arenas)
        versions = [devs[k]._version for k in (0, 2, 3)]
        if which == "capi":
            run_capi(torch, pkg.lib(), L, arenas, devs, grads)
        else:
            run_op(torch, ops, arenas, devs, grads)
            # the op advances the in-place version of what it mutates
            assert all(devs[k]._version > v for k, v in zip((0, 2, 3), versions))
        runs.append([d.cpu().numpy() for d in devs])
    for a, b, c in zip(*runs):
        assert np.array_equal(oc.bits(a), oc.bits(b)) and np.array_equal(oc.bits(b), oc.bits(c))
    run_host(pkg.lib(), L, arenas, grads)
    for a, got in zip(arenas, runs[1]):
        assert np.array_equal(oc.bits(a.host), oc.bits(got))


# ------------------------------------------------------------------------------ metrics
def host_metrics(lib, labels, pred, C, cm, counts):
    assert lib.pn2cpu_seg_confusion(oc.host_base(labels), oc.host_base(pred), len(labels), C,
                                    oc.host_base(cm), oc.host_base(counts)) == 0


def host_iou(lib, cm):
    C = cm.shape[0]
    iou, per = np.zeros(1, np.float32), np.zeros(C, np.float32)
    assert lib.pn2cpu_mean_iou(oc.host_base(cm), C, oc.host_base(iou), oc.host_base(per)) == 0
    return iou, per


@pytest.mark.parametrize("C", [2, 21, 64])
def test_confusion_and_mean_iou_equal_host_twins(env, C):
    pkg, ops, torch, dev, L = env
    lib = pkg.lib()
    R = L.PN2_CONFUSION_BLOCK_ROWS
    rng = np.random.default_rng(50 + C)
    for rows in (1, 63, 64, 65, R - 1, R, R + 1, 16 * 256 + 1):
        la, pa = oc.confusion_inputs(rng, rows, C)
        lb, pb = oc.confusion_inputs(rng, rows, C)
        cm, counts = np.zeros((C, C), np.int64), np.zeros(2, np.int64)
        runs = []
        for _ in range(2):
            dcm = torch.zeros(C, C, dtype=torch.int64, device=dev)
            dcounts = torch.zeros(2, dtype=torch.int64, device=dev)
            for lab, prd in ((la, pa), (lb, pb)):  # the second call accumulates
                ops.seg_confusion(torch.from_numpy(lab).to(dev), torch.from_numpy(prd).to(dev),
                                  dcm, dcounts)
            iou, per = ops.mean_iou(dcm)
            runs.append((dcm.cpu().numpy(), dcounts.cpu().numpy(), iou.cpu().numpy(),
                         per.cpu().numpy()))
        host_metrics(lib, la, pa, C, cm, counts)
        host_metrics(lib, lb, pb, C, cm, counts)
        hiou, hper = host_iou(lib, cm)
        for got in runs:
            assert np.array_equal(got[0], cm) and np.array_equal(got[1], counts), rows
            assert oc.bits(got[2].reshape(1)) == oc.bits(hiou), rows
            assert np.array_equal(oc.bits(got[3]), oc.bits(hper)), rows
        want_cm = oc.numpy_confusion(la, pa, C)[0] + oc.numpy_confusion(lb, pb, C)[0]
        assert np.array_equal(cm, want_cm)


def test_metrics_edge_cases(env):
    pkg, ops, torch, dev, L = env
    C = 21
    metrics = pkg.train.SegMetrics(C, device=dev)
    # an all-unannotated batch: nothing assigned, mean 0, accuracy NaN
    counts = metrics.update(torch.zeros(2, 50, dtype=torch.int64, device=dev),
                            torch.ones(2, 50, dtype=torch.int32, device=dev))
    assert counts.tolist() == [0, 0] and np.isnan(metrics.accuracy(counts))
    mean, per = metrics.iou()
    assert float(mean) == 0 and not per.any() and int(metrics.confusion.sum()) == 0
    # labels and predictions out of range are never used as an index; class 20 never occurs
    labels = torch.tensor([0, 1, 1, 2, 21, -1, 3, 3, 100, 5], dtype=torch.int32, device=dev)
    pred = torch.tensor([1, 1, 2, 2, 1, 1, 3, -1, 1, 21], dtype=torch.int32, device=dev)
    counts = metrics.update(labels, pred)
    assert counts.tolist() == [3, 4] and metrics.accuracy(counts) == 0.75  # 4 rows pass, 3 agree
    want = np.zeros((C, C), np.int64)
    for l, p in ((1, 1), (1, 2), (2, 2), (3, 3)):
        want[l, p] += 1
    assert np.array_equal(metrics.confusion.cpu().numpy(), want)
    mean, per = metrics.iou()
    mean64, per64 = oc.numpy_iou(want)   # classes 1, 2, 3: 1/2, 1/2, 1
    assert np.float32(mean64) == mean.cpu().numpy() and abs(mean64 - 2 / 3) < 1e-12
    assert np.array_equal(per.cpu().numpy(), per64.astype(np.float32)) and float(per[20]) == 0
    metrics.reset()
    assert int(metrics.confusion.sum()) == 0


# ------------------------------------------------------------------------------ the optimiser
B, N, NPOINT, RADIUS, NS = 2, 256, 64, 0.2, 16
SA_MLP, FP_MLP = [32, 64], [64, 32]


@functools.lru_cache(maxsize=None)
def small_cloud():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    xyz, feats = pkg.synth.batch([0, 1], N, "scannet", with_features=True)
    g = torch.Generator().manual_seed(3)
    labels = torch.randint(0, 4, (B, N), generator=g, dtype=torch.int32)
    return (torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(feats).to("cuda:0"),
            labels.to("cuda:0"))


def small_model(pkg, store, xyz, feats, is_training, extra=False):
    """One SA module, one FP module and a 4-class head."""
    pu, tu = pkg.pointnet_util, pkg.tf_util
    new_xyz, sa, _ = pu.pointnet_sa_module(xyz, feats, NPOINT, RADIUS, NS, SA_MLP, None, False,
                                           is_training, None, "sa1", params=store)
    fp = pu.pointnet_fp_module(xyz, new_xyz, feats, sa, FP_MLP, is_training, None, "fp1",
                               params=store)
    if extra:
        fp = tu.conv1d(fp, 32, 1, "extra", bn=True, is_training=is_training, params=store)
    return tu.conv1d(fp, 4, 1, "fc2", activation_fn=None, is_training=is_training, params=store)


def test_adam_optimizer_on_a_trainable_store(env):
    pkg, ops, torch, dev, L = env
    tu = pkg.tf_util
    xyz, feats, labels = small_cloud()
    store = tu.ParamStore(seed=9).trainable(dev)
    opt = pkg.train.AdamOptimizer(store, learning_rate=1e-2)   # before any variable exists
    loss = tu.sparse_softmax_cross_entropy(labels, small_model(pkg, store, xyz, feats, True))
    with torch.no_grad():
        before = small_model(pkg, store, xyz, feats, False).clone()
    loss.backward()
    names = [k for k, v in store.items() if v.requires_grad]
    assert len(names) == 4 * 4 + 2 and all(store[k].grad is not None for k in names)
    old = {k: (store[k].detach().clone(), store[k]._version) for k in names}
    opt.step()
    assert opt.t == 1
    for k in names:
        has_grad = float(store[k].grad.abs().max()) > 0
        # (a bias in front of a batch norm has no gradient: the batch mean takes it out)
        assert has_grad or (k.endswith("/biases") and k != "fc2/biases"), k
        if has_grad:
            assert not torch.equal(store[k].detach(), old[k][0]), k
        assert store[k]._version > old[k][1], k
        # the first step moves an element by at most the learning rate (plus half an ulp of
        # the parameter, |p| < 2)
        moved = (store[k].detach() - old[k][0]).abs().max()
        assert float(moved) <= 1e-2 + 2.5e-7, k
    with torch.no_grad():
        after = small_model(pkg, store, xyz, feats, False)   # no store.invalidate()
        fresh = small_model(pkg, tu.ParamStore(store.state_dict()), xyz, feats, False)
    assert not torch.equal(after, before) and torch.equal(after, fresh)
    # the optimiser's state is the twin's: one ApplyAdam from zero slots
    sd = opt.state_dict()
    k = "fc2/weights"
    g = store[k].grad.cpu().numpy()
    p2, m2, v2 = oc.numpy_adam(old[k][0].cpu().numpy(), g, np.zeros_like(g), np.zeros_like(g),
                               oc.alpha_of(1, lr=1e-2), oc.BETA1, oc.BETA2, oc.EPSILON,
                               np.float32)
    assert np.array_equal(oc.bits(sd[f"{k}/Adam"]), oc.bits(m2))
    assert np.array_equal(oc.bits(sd[f"{k}/Adam_1"]), oc.bits(v2))
    assert np.array_equal(oc.bits(store[k].detach().cpu().numpy()), oc.bits(p2))
    # a variable created after construction gets slots at the next step; a parameter without
    # a gradient is skipped, its slots untouched
    opt.zero_grad()
    assert all(store[k].grad is None for k in names)
    loss = tu.sparse_softmax_cross_entropy(labels, small_model(pkg, store, xyz, feats, True,
                                                               extra=True))
    loss.backward()
    store["sa1/conv0/weights"].grad = None
    kept = store["sa1/conv0/weights"].detach().clone()
    opt.step()
    sd2 = opt.state_dict()
    assert opt.t == 2 and sd2["global_step"] == 2
    for k in ("extra/weights", "extra/biases", "extra/bn/gamma", "extra/bn/beta"):
        assert sd2[f"{k}/Adam"].shape == tuple(store[k].shape), k
    assert sd2["extra/weights/Adam"].any() and sd2["extra/weights/Adam_1"].any()
    assert torch.equal(store["sa1/conv0/weights"].detach(), kept)
    assert np.array_equal(sd2["sa1/conv0/weights/Adam"], sd["sa1/conv0/weights/Adam"])


# ------------------------------------------------------------------------------ train_step
@functools.lru_cache(maxsize=None)
def cloud():
    import torch
    pkg = importlib.import_module(PKG_NAME)
    xyz, feats = pkg.synth.batch([0, 1], 1024, "scannet", with_features=True)
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, 4, (2, 1024), generator=g, dtype=torch.int32).to("cuda:0")
    w = (torch.rand(2, 1024, generator=g) * 4.5 + 0.5)
    w[labels.cpu() == 0] = 0.0
    return (torch.from_numpy(xyz).to("cuda:0"), torch.from_numpy(feats).to("cuda:0"), labels,
            w.to("cuda:0"))


def five_steps(pkg, torch):
    xyz, feats, labels, smpw = cloud()
    store = pkg.tf_util.ParamStore(seed=1).trainable("cuda:0")
    opt, metrics = pkg.train.AdamOptimizer(store), pkg.train.SegMetrics(4)
    losses, counts = [], []
    for i in range(5):
        loss, c = pkg.train.train_step(store, opt, metrics, xyz, labels, smpw, 4, bn_decay=0.5,
                                       learning_rate=pkg.train.get_learning_rate(i),
                                       features=feats, seed=100 + i)
        assert loss.is_cuda and c.is_cuda and not loss.requires_grad
        losses.append(loss)
        counts.append(c)
    return (torch.stack(losses).cpu().numpy(), store.state_dict(), opt.state_dict(),
            metrics.confusion.cpu().numpy(), torch.stack(counts).cpu().numpy(),
            [t.cpu().numpy() for t in metrics.iou()])


def test_five_train_steps_are_reproducible(env):
    pkg, ops, torch, dev, L = env
    a, b = five_steps(pkg, torch), five_steps(pkg, torch)
    losses, weights, state, cm, counts, (mean, per) = a
    assert np.array_equal(oc.bits(losses), oc.bits(b[0]))
    for x, y in ((weights, b[1]), (state, b[2])):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    assert np.array_equal(cm, b[3]) and np.array_equal(counts, b[4])
    assert np.array_equal(oc.bits(mean.reshape(1)), oc.bits(b[5][0].reshape(1)))
    assert np.array_equal(oc.bits(per), oc.bits(b[5][1]))
    print("train_step losses:", losses)
    assert np.isfinite(losses).all() and losses[4] < losses[0]
    assert state["global_step"] == 5
    assert sorted(k[:-5] for k in state if k.endswith("/Adam")) == sorted(
        k for k in weights if not k.endswith(("moving_mean", "moving_variance")))
    labels = cloud()[2].cpu().numpy()
    assigned = int(((labels > 0) & (labels < 4)).sum())
    assert (counts[:, 1] == assigned).all() and cm.sum() == 5 * assigned
    assert (counts[:, 0] <= counts[:, 1]).all() and np.trace(cm) == counts[:, 0].sum()
    mean64, per64 = oc.numpy_iou(cm)
    assert np.float32(mean64) == mean and np.array_equal(per64.astype(np.float32), per)


# ------------------------------------------------------------------------------ the models
def by_hand(pkg, xyz, l0_points, store):
    """pointnet2_sem_seg(_features).get_model with is_training=False as its module calls
    (pointnet2_sem_seg.py:29-59, pointnet2_sem_seg_features.py:25-57)."""
    pu, tu = pkg.pointnet_util, pkg.tf_util
    sa, fp = pu.pointnet_sa_module, pu.pointnet_fp_module
    l1_xyz, l1_p, _ = sa(xyz, l0_points, 1024, 0.1, 32, [32, 32, 64], None, False, False, None,
                         "layer1", params=store)
    l2_xyz, l2_p, _ = sa(l1_xyz, l1_p, 256, 0.2, 32, [64, 64, 128], None, False, False, None,
                         "layer2", params=store)
    l3_xyz, l3_p, _ = sa(l2_xyz, l2_p, 64, 0.4, 32, [128, 128, 256], None, False, False, None,
                         "layer3", params=store)
    l4_xyz, l4_p, _ = sa(l3_xyz, l3_p, 16, 0.8, 32, [256, 256, 512], None, False, False, None,
                         "layer4", params=store)
    l3_p = fp(l3_xyz, l4_xyz, l3_p, l4_p, [256, 256], False, None, "fa_layer1", params=store)
    l2_p = fp(l2_xyz, l3_xyz, l2_p, l3_p, [256, 256], False, None, "fa_layer2", params=store)
    l1_p = fp(l1_xyz, l2_xyz, l1_p, l2_p, [256, 128], False, None, "fa_layer3", params=store)
    l0_p = fp(xyz, l1_xyz, l0_points, l1_p, [128, 128, 128], False, None, "fa_layer4",
              params=store)
    feats = tu.conv1d(l0_p, 128, 1, "fc1", bn=True, is_training=False, params=store)
    return tu.conv1d(feats, 4, 1, "fc2", activation_fn=None, params=store), feats


def test_models_equal_their_module_calls(env):
    pkg, ops, torch, dev, L = env
    xyz, feats, _, _ = cloud()
    assert feats.shape == (2, 1024, 6)
    store = pkg.tf_util.ParamStore(seed=2)
    net, end_points = pkg.pointnet2_sem_seg_features.get_model(xyz, feats, False, 4, params=store)
    want, want_feats = by_hand(pkg, xyz, feats, store)
    assert net.shape == (2, 1024, 4) and end_points["l0_xyz"] is xyz
    assert torch.equal(net, want) and torch.equal(end_points["feats"], want_feats)
    assert tuple(store["layer1/conv0/weights"].shape) == (1, 1, 9, 32)
    assert tuple(store["fa_layer4/conv_0/weights"].shape) == (1, 1, 134, 128)
    # the model without features, from the same body: unchanged
    plain = pkg.tf_util.ParamStore(seed=2)
    net0, end0 = pkg.pointnet2_sem_seg.get_model(xyz, False, 4, params=plain)
    want0, want_feats0 = by_hand(pkg, xyz, None, plain)
    assert torch.equal(net0, want0) and torch.equal(end0["feats"], want_feats0)
    assert tuple(plain["layer1/conv0/weights"].shape) == (1, 1, 3, 32)
    assert not torch.equal(net0, net)
