"""MI355X: the kernels of csrc/feed.hip and pn2_val_select (csrc/scene.hip) against their host
twins (csrc/cpu_feed.cpp) bit for bit, the three new operators under the Meta key against the
device, the three attention models against their module calls, one training step per model, and
three steps of train() with one eval_model end to end. tests/test_feed_cpu.py pins the twins to
the reference's own outputs and to numpy."""
import importlib
import json
import math
import os

import numpy as np
import pytest

import feed_cases as fc
import support

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FEED_GRID_ROWS = 1024 * 256  # kFeedMaxBlocks * kBlock (csrc/feed.hip): rows past it are strided


@pytest.fixture(scope="module")
def env():
    import torch

    import pn2hip
    pkg = importlib.import_module(fc.PKG_NAME)
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def same_bits(torch, got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.is_cuda and not w.is_cuda, k
        assert (g.shape, g.dtype) == (w.shape, w.dtype), k
        support.same_bits(g, w, k)


# ------------------------------------------------------------------ feed_batch
def feed_args(torch, B, N, use_color, use_normal, rotate, seed=0):
    g = np.random.default_rng(seed)
    t = torch.from_numpy
    pts = t(g.normal(0, 3, (B, N, 3)).astype(np.float32))
    lab = t(g.integers(-1, 23, (B, N)).astype(np.int32))
    col = t(g.integers(-3, 260, (B, N, 3)).astype(np.int32))
    nrm = t(g.normal(0, 1, (B, N, 3)).astype(np.float32))
    sw = t(g.choice(np.array([0.0, -0.0, np.nan, 1e-30, 1.0], np.float32), (B, N)))
    pkg = importlib.import_module(fc.PKG_NAME)
    cs = t(pkg.rotation_cs(g.uniform(0, 2 * math.pi, B))) if rotate else None
    cw = torch.tensor(pkg.CLASS_WEIGHTS, dtype=torch.float32)
    return [pts, lab, col if use_color else None, nrm if use_normal else None, sw, cs, cw,
            use_color, use_normal]


def on(dev, args):
    return [a.to(dev) if hasattr(a, "to") else a for a in args]


@pytest.mark.parametrize("B,N", [(1, 1), (2, 63), (3, 257)])
@pytest.mark.parametrize("use_color", [False, True])
@pytest.mark.parametrize("use_normal", [False, True])
@pytest.mark.parametrize("rotate", [False, True])
def test_feed_batch_kernel_equals_twin(env, B, N, use_color, use_normal, rotate):
    pkg, ops, torch, dev = env
    args = feed_args(torch, B, N, use_color, use_normal, rotate, seed=B)
    same_bits(torch, ops.feed_batch(*on(dev, args)), ops.feed_batch(*args))


def test_feed_batch_past_the_grid(env):
    """More rows than one pass of the grid: the stride loop runs, with rows of three clouds."""
    pkg, ops, torch, dev = env
    N = (FEED_GRID_ROWS + 77 * 3) // 3
    assert 3 * N > FEED_GRID_ROWS and (3 * N) % 256
    args = feed_args(torch, 3, N, True, True, True, seed=9)
    same_bits(torch, ops.feed_batch(*on(dev, args)), ops.feed_batch(*args))


def test_feed_batch_offset_and_strided_inputs(env):
    """A contiguous view 4 bytes into its buffer (16-byte misaligned) is read in place; a strided
    view is made contiguous by the operator. Same bits as the aligned call."""
    pkg, ops, torch, dev = env
    args = feed_args(torch, 2, 63, True, True, True, seed=4)
    want = ops.feed_batch(*args)
    d = on(dev, args)

    def offset(a):
        buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=dev)
        v = buf[1:].view(a.shape)
        v.copy_(a)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    def strided(a):
        wide = torch.zeros(a.shape[:-1] + (2 * a.shape[-1],), dtype=a.dtype, device=dev)
        v = wide[..., ::2]
        v.copy_(a)
        assert not v.is_contiguous()
        return v
    for make, idxs in ((offset, (0, 1, 2, 3, 4, 5, 6)), (strided, (0, 2, 3, 1, 4))):
        a = list(d)
        for k in idxs:
            a[k] = make(d[k])
        same_bits(torch, ops.feed_batch(*a), want)


def test_random_rotate_and_get_data_tensors_on_the_device(env):
    pkg, ops, torch, dev = env
    args = feed_args(torch, 2, 63, True, True, False, seed=6)
    pts, lab, col, nrm, sw = args[:5]
    alpha = [0.25, 4.0]
    got = pkg.random_rotate(pts.to(dev), lab.to(dev), col.to(dev), nrm.to(dev), sw.to(dev), alpha)
    want = pkg.random_rotate(pts, lab, col, nrm, sw, alpha)
    same_bits(torch, (got[0], got[3]), (want[0], want[3]))
    got = pkg.get_data_tensors((pts, lab, col, nrm, sw), True, True, dev)
    want = pkg.get_data_tensors((pts, lab, col, nrm, sw), True, True, "cpu")
    same_bits(torch, got, want)


# ------------------------------------------------------------------ the validation chunker
@pytest.fixture(scope="module")
def scenes(env):
    """name -> (points, labels, colors, normals) CPU tensors, made once and never written to."""
    pkg, ops, torch, dev = env
    synth = pkg.synth
    out = {"n3000": synth.scannet_scene(7, 3000),    # one selection slice, 3000 % 256 != 0
           "n6000": synth.scannet_scene(8, 6000),    # two slices (4096 + 1904), 6000 % 256 != 0
           "skip_path": fc.skip_path_scene()}
    small = synth.scannet_scene(9, 700)
    out["one_column"] = ((small[0] * np.float32(0.2)),) + tuple(small[1:])  # 1.2 m x 0.9 m
    return {k: tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in v) for k, v in out.items()}


def select(env, scene, dev):
    pkg, ops, torch, _ = env
    P = scene[0].to(dev)
    bounds = torch.from_numpy(pkg.data_transformation._val_bounds(scene[0])).to(dev)
    return ops.val_select(P, bounds, 0.2, 0.001)


def chunks(env, scene, sel3, dev, choice, u, K, min_inside=0.01):
    pkg, ops, torch, _ = env
    mv = lambda a: None if a is None else a.to(dev)  # noqa: E731
    lw = torch.ones(21)
    lw[0] = 0
    return ops.val_chunks(*[mv(a) for a in scene], *[mv(a) for a in sel3], mv(choice), mv(u), K,
                          mv(lw), min_inside)


@pytest.mark.parametrize("name", ["n3000", "n6000", "skip_path", "one_column"])
def test_val_select_kernel_equals_twin(env, scenes, name):
    pkg, ops, torch, dev = env
    got, want = select(env, scenes[name], dev), select(env, scenes[name], "cpu")
    counts = want[0]
    assert got[0].dtype == torch.int32 and torch.equal(got[0].cpu(), counts)
    assert len(counts) == (1 if name == "one_column" else 20)
    # sel and inner are defined up to each column's count
    for s, n in enumerate(counts.tolist()):
        assert torch.equal(got[1][s, :n].cpu(), want[1][s, :n]), s
        assert torch.equal(got[2][s, :n].cpu(), want[2][s, :n]), s


def skip_choice(torch, counts, inner, K, skip, seed):
    """(S, K) draws: columns in `skip` draw only points outside the inner box (drawn for, then
    skipped), the others draw among all of their points."""
    g = np.random.default_rng(seed)
    choice = np.zeros((len(counts), K), np.int32)
    for s, n in enumerate(counts.tolist()):
        if n == 0:
            continue
        pool = np.arange(n)
        if s in skip:
            pool = np.nonzero(inner[s, :n].numpy() == 0)[0]
            assert len(pool), s
        choice[s] = g.choice(pool, K)
    return torch.from_numpy(choice)


@pytest.mark.parametrize("name,K,skip", [
    ("n3000", 200, ()), ("n3000", 257, (0, 19)), ("n6000", 256, (0, 7, 19)), ("n6000", 257, (9,)),
    ("skip_path", 256, ()), ("skip_path", 200, (19,)), ("one_column", 257, ())])
def test_val_chunks_kernel_equals_twin(env, scenes, name, K, skip):
    """Skipped columns first, in the middle and last in column order; npoints below, at and past
    the workgroup size; the choice path and the u path; two streams."""
    pkg, ops, torch, dev = env
    scene = scenes[name]
    sel_h = select(env, scene, "cpu")
    sel_d = select(env, scene, dev)
    # the device's own selection feeds the device's chunks; rows past the counts are undefined in
    # both, so the twin gets the device's buffers: equal where defined (the test above)
    sel_dh = tuple(t.cpu() for t in sel_d)
    counts = sel_h[0]
    choice = skip_choice(torch, counts, sel_h[2], K, set(skip), seed=K)
    want = chunks(env, scene, sel_dh, "cpu", choice, None, K)
    got = chunks(env, scene, sel_d, dev, choice, None, K)
    same_bits(torch, got, want)
    column, kept = want[5].tolist(), int(want[6])
    inner_h = sel_h[2].numpy()
    expect = [s for s, n in enumerate(counts.tolist())
              if n and not inner_h[s][choice[s].numpy()].sum() / float(K) < 0.01]
    assert column[:kept] == expect and not set(skip) & set(expect)
    assert column[kept:] == [-1] * (len(counts) - kept)
    if name == "skip_path":  # two empty columns, and (1,1) with no point inside
        assert not {5, 12, 16} & set(expect) and counts[12] == counts[16] == 0
    # the u path
    u = torch.rand((len(counts), K), generator=torch.Generator().manual_seed(K))
    same_bits(torch, chunks(env, scene, sel_d, dev, None, u, K),
              chunks(env, scene, sel_dh, "cpu", None, u, K))
    # the same call on two streams: the same bits
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            outs.append(chunks(env, scene, sel_d, dev, choice, None, K))
        st.synchronize()
    for a, b, c in zip(outs[0], outs[1], got):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_every_column_skipped(env, scenes, monkeypatch):
    pkg, ops, torch, dev = env
    scene = scenes["n3000"]
    sel_d = select(env, scene, dev)
    u = torch.rand((20, 200), generator=torch.Generator().manual_seed(1))
    got = chunks(env, scene, sel_d, dev, None, u, 200, min_inside=1.5)
    want = chunks(env, scene, tuple(t.cpu() for t in sel_d), "cpu", None, u, 200, min_inside=1.5)
    same_bits(torch, got, want)
    assert int(got[6]) == 0 and got[5].tolist() == [-1] * 20 and not got[0].any()
    dt = pkg.data_transformation
    monkeypatch.setattr(dt, "VAL_MIN_INSIDE", 1.5)
    assert dt.scene_val_chunks(*[a.to(dev) for a in scene], 200, u=u)[0].shape == (0, 200, 3)
    with pytest.raises(ValueError, match="need at least one array to concatenate"):
        dt.get_all_subsets_for_scene_numpy(*[a.numpy() for a in scene], 200)


@pytest.mark.parametrize("case", fc.GOLDEN_CASES, ids=[c[0] for c in fc.GOLDEN_CASES])
def test_numpy_chunker_on_the_device_equals_the_reference(env, case):
    pkg, ops, torch, dev = env
    name, sid, n, npoints, seed = case
    gold = {g["name"]: g for g in json.load(open(os.path.join(HERE, "golden", "val_chunks.json")))}
    np.random.seed(seed)
    res = pkg.data_transformation.get_all_subsets_for_scene_numpy(*fc.golden_scene(name, sid, n),
                                                                  npoints)
    for key, a in zip(fc.OUTPUT_NAMES, res):
        assert fc.digest(a) == gold[name]["outputs"][key], key


# ------------------------------------------------------------------ Meta
def meta_table(torch, dev):
    gen = torch.Generator().manual_seed(0)
    f = lambda *s: torch.rand(s, generator=gen).to(dev)  # noqa: E731
    i = lambda hi, *s: torch.randint(0, hi, s, generator=gen, dtype=torch.int32).to(dev)  # noqa: E731
    N, S, K = 50, 3, 8
    bounds = torch.tensor([[0, 0, 0, .5, .5, 1], [.5, 0, 0, 1, .5, 1], [2, 2, 2, 3, 3, 3]],
                          dtype=torch.float64, device=dev)
    pts = f(N, 3)
    return {
        "feed_batch": (f(2, 9, 3), i(21, 2, 9), i(255, 2, 9, 3), f(2, 9, 3), f(2, 9), f(2, 2),
                       f(21), True, True),
        "feed_batch-plain": (f(2, 9, 3), i(21, 2, 9), None, None, f(2, 9), None, f(21), False,
                             False),
        "feed_batch-empty": (f(0, 9, 3), i(21, 0, 9), None, None, f(0, 9), None, f(21), False,
                             False),
        "val_select": (pts, bounds, 0.2, 0.001),
        "val_chunks": lambda sel: (pts, i(21, N), i(255, N, 3), None, *sel, None, f(S, K), K,
                                   f(21), 0.01),
        "val_chunks-choice": lambda sel: (pts, i(21, N), None, f(N, 3), *sel, i(N, S, K), None, K,
                                          f(21), 0.01),
    }


@pytest.mark.parametrize("case", ["feed_batch", "feed_batch-plain", "feed_batch-empty",
                                  "val_select", "val_chunks", "val_chunks-choice"])
def test_meta_agrees_with_the_device(env, case):
    pkg, ops, torch, dev = env
    table = meta_table(torch, dev)
    args = table[case]
    if callable(args):
        args = args(ops.val_select(*table["val_select"]))
    op = getattr(ops, case.split("-")[0])
    meta = tuple(a.to("meta") if isinstance(a, torch.Tensor) else a for a in args)
    got, want = op(*meta), op(*args)
    torch.cuda.synchronize()
    assert type(got) is type(want) and len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.is_meta and w.is_cuda, k
        assert (g.shape, g.dtype, g.stride()) == (w.shape, w.dtype, w.stride()), k


# ------------------------------------------------------------------ the models
B, N, NCLS = 2, 2048, 21
MODELS = ("attention", "attention_and_pooling", "single_layer")
SINGLE_IDX = 2


@pytest.fixture(scope="module")
def cloud(env):
    pkg, ops, torch, dev = env
    xyz, _ = pkg.synth.batch([0, 1], N, "scannet")
    g = torch.Generator().manual_seed(5)
    labels = torch.randint(0, NCLS, (B, N), generator=g, dtype=torch.int32)
    w = torch.rand(B, N, generator=g) * 4.5 + 0.5
    w[labels == 0] = 0.0
    return torch.from_numpy(xyz).to(dev), labels.to(dev), w.to(dev)


def model_of(pkg, name):
    """(get_model(xyz, is_training, params), body, the SA module of each layer)."""
    al, pu = pkg.attention_layer, pkg.pointnet_util
    att, pool, sa = al.pointnet_sa_module_attention, al.pointnet_sa_module_attention_and_pooling, \
        pu.pointnet_sa_module
    if name == "attention":
        m = pkg.pointnet2_sem_seg_attention
        return (lambda x, t, s: m.get_model(x, t, NCLS, params=s)), m.body, (att,) * 4
    if name == "attention_and_pooling":
        m = pkg.pointnet2_sem_seg_attention_and_pooling
        return (lambda x, t, s: m.get_model(x, t, NCLS, params=s)), m.body, (pool,) * 4
    m = pkg.pointnet2_sem_seg_attention_single_layer
    mods = tuple(att if k == SINGLE_IDX else sa for k in range(4))
    return (lambda x, t, s: m.get_model(x, SINGLE_IDX, t, NCLS, params=s)), m.body(SINGLE_IDX), mods


def by_hand(pkg, xyz, store, mods):
    """The reference's get_model with is_training=False as its module calls
    (pointnet2_sem_seg_attention.py:28-60 and its two siblings)."""
    pu, tu = pkg.pointnet_util, pkg.tf_util
    fp = pu.pointnet_fp_module
    l1_xyz, l1_p, _ = mods[0](xyz, None, 1024, 0.1, 32, [32, 32, 64], None, False, False, None,
                              "layer1", params=store)
    l2_xyz, l2_p, _ = mods[1](l1_xyz, l1_p, 256, 0.2, 32, [64, 64, 128], None, False, False, None,
                              "layer2", params=store)
    l3_xyz, l3_p, _ = mods[2](l2_xyz, l2_p, 64, 0.4, 32, [128, 128, 256], None, False, False, None,
                              "layer3", params=store)
    l4_xyz, l4_p, _ = mods[3](l3_xyz, l3_p, 16, 0.8, 32, [256, 256, 512], None, False, False, None,
                              "layer4", params=store)
    l3_p = fp(l3_xyz, l4_xyz, l3_p, l4_p, [256, 256], False, None, "fa_layer1", params=store)
    l2_p = fp(l2_xyz, l3_xyz, l2_p, l3_p, [256, 256], False, None, "fa_layer2", params=store)
    l1_p = fp(l1_xyz, l2_xyz, l1_p, l2_p, [256, 128], False, None, "fa_layer3", params=store)
    l0_p = fp(xyz, l1_xyz, None, l1_p, [128, 128, 128], False, None, "fa_layer4", params=store)
    feats = tu.conv1d(l0_p, 128, 1, "fc1", bn=True, is_training=False, params=store)
    return tu.conv1d(feats, NCLS, 1, "fc2", activation_fn=None, params=store), feats


@pytest.mark.parametrize("name", MODELS)
def test_models_equal_their_module_calls(env, cloud, name):
    pkg, ops, torch, dev = env
    xyz = cloud[0]
    get_model, _, mods = model_of(pkg, name)
    store = pkg.tf_util.ParamStore(seed=2)
    net, end_points = get_model(xyz, False, store)
    want, want_feats = by_hand(pkg, xyz, pkg.tf_util.ParamStore(seed=2), mods)
    assert net.shape == (B, N, NCLS) and end_points["l0_xyz"] is xyz
    assert torch.equal(net, want) and torch.equal(end_points["feats"], want_feats)
    att_layers = range(1, 5) if name != "single_layer" else (SINGLE_IDX + 1,)
    for k in range(1, 5):
        has = f"layer{k}/ScannetAttentionLayer/dense_2/kernel" in store
        assert has == (k in att_layers), k
        assert (f"layer{k}/layer{k}/gamma" in store) == (k in att_layers), k
        assert f"layer{k}/conv2/weights" in store
    assert "fa_layer4/conv_2/weights" in store and "fc2/biases" in store


def one_step(pkg, torch, cloud, name, seed):
    xyz, labels, smpw = cloud
    _, body, _ = model_of(pkg, name)
    store = pkg.tf_util.ParamStore(seed=1).trainable("cuda:0")
    with torch.no_grad():  # create every variable, then remember it
        body(xyz, None, False, NCLS, None, store)
    before = store.state_dict()
    opt, metrics = pkg.train.AdamOptimizer(store), pkg.train.SegMetrics(NCLS)
    loss, counts = pkg.train.train_step_with(body, store, opt, metrics, xyz, labels, smpw, NCLS,
                                             bn_decay=0.5, learning_rate=1e-3, seed=seed)
    assert loss.is_cuda and counts.is_cuda and not loss.requires_grad
    return before, store, float(loss), store.state_dict()


@pytest.mark.parametrize("name", MODELS)
def test_one_train_step_moves_every_variable_and_repeats(env, cloud, name):
    pkg, ops, torch, dev = env
    before, store, loss, after = one_step(pkg, torch, cloud, name, seed=11)
    assert math.isfinite(loss)
    trainable = [k for k, v in store.items() if v.requires_grad]
    dense = [k for k in trainable if "ScannetAttentionLayer" in k and k.endswith("kernel")]
    assert len(dense) == (3 if name == "single_layer" else 12)
    for k in trainable:
        # a conv bias in front of a batch norm has no gradient (the batch mean takes it out), so
        # Adam leaves it where it is; every other variable must move
        if k.endswith("/biases") and k != "fc2/biases":
            continue
        assert not np.array_equal(before[k], after[k]), k
    _, _, loss2, after2 = one_step(pkg, torch, cloud, name, seed=11)
    assert loss2 == loss and set(after2) == set(after)
    for k in after:
        assert np.array_equal(fc.bits(after[k]), fc.bits(after2[k])), k


# ------------------------------------------------------------------ the loop, end to end
READS = ("item", "tolist", "cpu", "numpy", "__bool__", "__float__", "__int__", "__index__")


def test_train_and_eval_model_end_to_end_without_reading_back_inside_a_step(env, monkeypatch):
    """Three steps of train() (one epoch of three batches, then validation on two chunks of a
    scene's validation chunker) through get_data_tensors, train_step and eval_step. While a step
    runs, every way Python reads a device tensor back (and torch.cuda.synchronize) is counted:
    none may happen."""
    pkg, ops, torch, dev = env
    tr = pkg.train
    scene = fc.golden_scene("scene1", 1, 20000)
    p, l, c, n, w = pkg.scene_val_chunks(*[torch.from_numpy(a).to(dev) for a in scene], 2048,
                                         generator=torch.Generator(dev).manual_seed(3))
    assert p.shape[0] >= 8
    stored = [tuple(t[2 * k:2 * k + 2] for t in (p, l, c, n, w)) for k in range(4)]
    reads, inside = [], [False]

    def counted(name, fn):
        def wrapper(self, *a, **k):
            if inside[0] and getattr(self, "is_cuda", False):
                reads.append(name)
            return fn(self, *a, **k)
        return wrapper
    for name in READS:
        monkeypatch.setattr(torch.Tensor, name, counted(name, getattr(torch.Tensor, name)))
    sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize",
                        lambda *a, **k: (reads.append("synchronize") if inside[0] else None,
                                         sync(*a, **k))[1])

    def guarded(fn):
        def run(*a, **k):
            inside[0] = True
            try:
                return fn(*a, **k)
            finally:
                inside[0] = False
        return run
    store = pkg.tf_util.ParamStore(seed=4).trainable(dev)
    hist = tr.train(store, stored[:3], stored[2:], epochs=1, batch_size=2, n_train_samples=6,
                    n_epochs_to_val=1,
                    step_fn=guarded(lambda *a, model=None, **k: tr.train_step_with(model, *a, **k)),
                    eval_fn=guarded(tr.eval_step),
                    device=dev, seed=50)
    assert reads == []
    assert len(hist) == 1 and hist[0]["epoch"] == 2 and hist[0]["step"] == 3
    h = hist[0]
    for key in ("loss", "accuracy", "iou", "val_loss", "val_accuracy", "val_iou"):
        assert math.isfinite(h[key]) and h[key] >= 0, key
    assert 0 <= h["iou"] <= 1 and 0 <= h["val_accuracy"] <= 1
    # eval_model alone: the same validation figures on the trained store, metrics reset after it
    vm = tr.SegMetrics(21, dev)
    vl, va, vi = tr.eval_model(store, vm, stored[2:], device=dev)
    assert (vl, va, vi) == (h["val_loss"], h["val_accuracy"], h["val_iou"])
    assert not vm.confusion.any()
