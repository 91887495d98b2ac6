"""CPU: the path from a stored scene to train_step through the host twins of csrc/feed.hip and
pn2_val_select (csrc/cpu_feed.cpp; the CPU kernels of torch.ops.pn2.feed_batch / val_select /
val_chunks): the validation chunker against tests/golden/val_chunks.json, which the reference's
own get_all_subsets_for_scene_numpy wrote (tests/golden/make_golden_val_chunks.py), feed_batch
against its numpy statement bit for bit, the class weights, the epoch loop with stub steps, and the
C ABI's guards. tests/test_gpu_feed.py compares the kernels with these twins on the MI355X."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import feed_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
E = -22
GOLD = {g["name"]: g for g in json.load(open(os.path.join(HERE, "golden", "val_chunks.json")))}
CASES = {c[0]: c for c in fc.GOLDEN_CASES}


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


@pytest.fixture(scope="module")
def scenes():
    """name -> the scene's arrays, made once and never written to."""
    return {name: fc.golden_scene(name, sid, n) for name, sid, n, _, _ in fc.GOLDEN_CASES}


def check_golden(name, res):
    g = GOLD[name]
    for key, a in zip(fc.OUTPUT_NAMES, res):
        assert fc.digest(a) == g["outputs"][key], (name, key)
        assert np.asarray(a)[0, :4].tolist() == g["head"][key], (name, key)


# ------------------------------------------------------------------ the validation chunker
@pytest.mark.parametrize("name", list(CASES))
def test_numpy_chunker_equals_the_reference(pn2, scenes, name):
    _, _, _, npoints, seed = CASES[name]
    np.random.seed(seed)
    res = pn2.data_transformation.get_all_subsets_for_scene_numpy(*scenes[name], npoints,
                                                                  device="cpu")
    assert [a.dtype for a in res] == [np.float32, np.int32, np.int32, np.float32, np.float64]
    check_golden(name, res)


def reference_choice(pn2, ops, pts, npoints, seed):
    """The reference's draws: np.random.choice per non-empty column, in column order."""
    dt = pn2.data_transformation
    P = torch.from_numpy(pts)
    bounds = torch.from_numpy(dt._val_bounds(P))
    counts = ops.val_select(P, bounds, 0.2, 0.001)[0].numpy()
    np.random.seed(seed)
    choice = np.zeros((len(counts), npoints), np.int32)
    for s, n in enumerate(counts):
        if n:
            choice[s] = np.random.choice(int(n), npoints, replace=True)
    return counts, choice


@pytest.mark.parametrize("name", list(CASES))
def test_scene_val_chunks_with_the_reference_draws(pn2, ops, scenes, name):
    _, _, _, npoints, seed = CASES[name]
    sc = scenes[name]
    _, choice = reference_choice(pn2, ops, sc[0], npoints, seed)
    res = pn2.scene_val_chunks(*(torch.from_numpy(a) for a in sc), npoints, choice=choice)
    assert all(isinstance(t, torch.Tensor) and t.device.type == "cpu" for t in res)
    assert res[4].dtype == torch.float32
    w64 = res[4].numpy().astype(np.float64)  # 0 and 1: exact in either format
    assert set(np.unique(w64)) <= {0.0, 1.0}
    check_golden(name, [t.numpy() for t in res[:4]] + [w64])


def test_skip_paths_are_the_ones_the_fixture_pins(pn2, ops, scenes):
    """Column (1,1) selects points, none of them inside: drawn for, then skipped. Columns (3,0)
    and (4,0) select nothing: no draw. 17 of 20 columns remain, in column order."""
    pts, lab, col, nrm = scenes["skip_path"]
    counts, choice = reference_choice(pn2, ops, pts, 256, 3)
    assert len(counts) == 20 and counts[1 * 4 + 1] == 369
    assert counts[3 * 4 + 0] == 0 and counts[4 * 4 + 0] == 0 and (counts > 0).sum() == 18
    P = torch.from_numpy(pts)
    c, sel, inner = ops.val_select(P, torch.from_numpy(pn2.data_transformation._val_bounds(P)),
                                   0.2, 0.001)
    assert int(inner[5, :369].sum()) == 0
    out = ops.val_chunks(P, torch.from_numpy(lab), torch.from_numpy(col), torch.from_numpy(nrm),
                         c, sel, inner, torch.from_numpy(choice), None, 256,
                         torch.ones(21), 0.01)
    column, kept = out[5].numpy(), int(out[6])
    assert kept == 17 and GOLD["skip_path"]["outputs"]["labels"]["shape"] == [17, 256]
    assert column.tolist() == [s for s in range(20) if s not in (5, 12, 16)] + [-1] * 3
    for t in out[:5]:  # the chunks past `kept` are zeroed
        assert not t[kept:].any()


def test_chunker_edges(pn2, ops):
    dt = pn2.data_transformation
    P = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    L = torch.tensor([0, 3], dtype=torch.int32)
    # one column; the u path: int(u * n), clamped
    u = torch.tensor([[0.0, 0.49, 0.5, 0.999, 1.0, -1.0]])
    p, l, c, n, w = dt.scene_val_chunks(P, L, None, None, 6, u=u)
    assert c is None and n is None and p.shape == (1, 6, 3)
    assert l[0].tolist() == [0, 0, 3, 3, 3, 0] and w[0].tolist() == [0, 0, 1, 1, 1, 0]
    # an out-of-range choice is clamped
    p, l, _, _, _ = dt.scene_val_chunks(P, L, None, None, 3, choice=np.array([[-5, 1, 7]]))
    assert l[0].tolist() == [0, 3, 3]
    # every column skipped: nothing inside (min_inside above 1), kept = 0
    c_, sel, inner = ops.val_select(P, torch.from_numpy(dt._val_bounds(P)), 0.2, 0.001)
    out = ops.val_chunks(P, L, None, None, c_, sel, inner, None, u, 6, torch.ones(21), 1.5)
    assert int(out[6]) == 0 and out[5].tolist() == [-1] and out[2].shape == (0,)
    with pytest.raises(ValueError, match="negative"):
        dt.get_all_subsets_for_scene_numpy(P.numpy(), L.numpy(), np.zeros((2, 3), np.int32),
                                           P.numpy(), -1, device="cpu")


def test_numpy_chunker_raises_when_every_column_is_skipped(pn2):
    """With every chunk dropped (a keep threshold no chunk can meet) the reference's
    np.concatenate of nothing raises ValueError; so does this."""
    dt = pn2.data_transformation
    pts = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]], np.float32)
    lab = np.zeros(2, np.int32)
    saved = dt.VAL_MIN_INSIDE
    dt.VAL_MIN_INSIDE = 1.5  # no chunk can have 150 % of its draws inside
    try:
        with pytest.raises(ValueError, match="need at least one array to concatenate"):
            dt.get_all_subsets_for_scene_numpy(pts, lab, np.zeros((2, 3), np.int32), pts, 8,
                                               device="cpu")
    finally:
        dt.VAL_MIN_INSIDE = saved


# ------------------------------------------------------------------ feed_batch
def feed_inputs(B, N, seed=0):
    g = np.random.default_rng(seed)
    pts = (g.normal(0, 3, (B, N, 3))).astype(np.float32)
    lab = g.integers(-1, 23, (B, N)).astype(np.int32)
    col = g.integers(0, 256, (B, N, 3)).astype(np.int32)
    nrm = g.normal(0, 1, (B, N, 3)).astype(np.float32)
    sw = g.choice(np.array([0.0, -0.0, np.nan, 1e-30, 1.0, 2.5], np.float32), (B, N))
    alpha = g.uniform(0, 2 * math.pi, B)
    return pts, lab, col, nrm, sw, alpha


def run_feed(ops, dev, pts, lab, col, nrm, sw, cs, cw, use_color, use_normal):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = ops.feed_batch(t(pts), t(lab), t(col), t(nrm), t(sw), t(cs), t(np.asarray(cw, np.float32)),
                         use_color, use_normal)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("use_color,use_normal", [(False, False), (True, False), (False, True),
                                                   (True, True)])
@pytest.mark.parametrize("rotate", [False, True])
def test_feed_batch_equals_its_numpy_statement(pn2, ops, use_color, use_normal, rotate):
    pts, lab, col, nrm, sw, alpha = feed_inputs(3, 257)
    cs = pn2.rotation_cs(alpha) if rotate else None
    cw = pn2.CLASS_WEIGHTS
    got = run_feed(ops, "cpu", pts, lab, col, nrm, sw, cs, cw, use_color, use_normal)
    want = fc.feed_batch_numpy(pts, lab, col, nrm, sw, cs, cw, use_color, use_normal)
    assert got[1].shape == (3, 257, 3 * use_color + 3 * use_normal)
    for g, w in zip(got, want):
        assert g.dtype == np.float32 and np.array_equal(fc.bits(g), fc.bits(w))
    if not rotate:
        assert np.array_equal(fc.bits(got[0]), fc.bits(pts))


def test_rotation_stays_within_the_two_products_one_sum_bound(pn2, ops):
    """x' = fl(fl(x c) + fl(y s)): each product errs by at most 2^-24 of itself and the sum by
    2^-24 of its result, so |x' - (x c + y s)| <= 2^-23 (|x c| + |y s|) up to second order, which
    the factor 1 + 2^-23 below covers; the same for y'."""
    g = np.random.default_rng(5)
    pts = g.normal(0, 4, (8, 4096, 3)).astype(np.float32)
    cs = pn2.rotation_cs(g.uniform(0, 2 * math.pi, 8))
    z = np.zeros((8, 4096), np.float32)
    xyz = run_feed(ops, "cpu", pts, z.astype(np.int32), None, None, z, cs, [], False, False)[0]
    x, y = pts[..., 0].astype(np.float64), pts[..., 1].astype(np.float64)
    c, s = cs[:, 0:1].astype(np.float64), cs[:, 1:2].astype(np.float64)
    tol = 2.0 ** -23 * (1 + 2.0 ** -23)
    assert (np.abs(xyz[..., 0] - (x * c + y * s)) <= tol * (np.abs(x * c) + np.abs(y * s))).all()
    assert (np.abs(xyz[..., 1] - (y * c - x * s)) <= tol * (np.abs(y * c) + np.abs(x * s))).all()
    assert np.array_equal(xyz[..., 2], pts[..., 2])
    # and it is a rotation: cos^2 + sin^2 = 1 to float32
    assert np.allclose(cs[:, 0].astype(np.float64) ** 2 + cs[:, 1].astype(np.float64) ** 2, 1,
                       atol=2e-7)


def test_colours_divide_correctly_rounded(ops):
    vals = np.concatenate([np.arange(0, 256), -np.arange(1, 300),
                           [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    vals = np.resize(vals, (1, 188, 3))
    z = np.zeros((1, 188), np.float32)
    feats = run_feed(ops, "cpu", np.zeros((1, 188, 3), np.float32), z.astype(np.int32), vals, None,
                     z, None, [], True, False)[1]
    want = vals.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(fc.bits(feats), fc.bits(want))
    # correctly rounded: the float32 nearest to the float64 quotient of the converted colour
    assert np.array_equal(feats, (vals.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32))


def test_sample_weights_mask_and_range(pn2, ops):
    labels = np.array([[-1, 0, 20, 21]], np.int32).repeat(4, 0).reshape(1, 16)
    stored = np.array([0.0, -0.0, np.nan, 1e-30], np.float32).repeat(4).reshape(1, 16)
    cw = pn2.CLASS_WEIGHTS
    smpw = run_feed(ops, "cpu", np.zeros((1, 16, 3), np.float32), labels, None, None, stored, None,
                    cw, False, False)[2].reshape(4, 4)
    w20 = np.float32(cw[20])
    assert not smpw[0].any() and not smpw[1].any()          # 0.0 and -0.0: mask 0
    for row in (smpw[2], smpw[3]):                          # NaN and 1e-30: mask 1
        assert row.tolist() == [0.0, 0.0, float(w20), 0.0]  # labels -1, 0 (weight 0), 20, 21


def test_random_rotate_and_get_data_tensors(pn2):
    pts, lab, col, nrm, sw, alpha = feed_inputs(2, 63, seed=2)
    t = [torch.from_numpy(a) for a in (pts, lab, col, nrm, sw)]
    rp, rl, rc, rn, rw = pn2.random_rotate(*t, alpha=alpha)
    cs = pn2.rotation_cs(alpha)
    want = fc.feed_batch_numpy(pts, lab, col, nrm, sw, cs, [], False, True)
    assert np.array_equal(fc.bits(rp.numpy()), fc.bits(want[0]))
    assert np.array_equal(fc.bits(rn.numpy()), fc.bits(want[1]))
    assert rl is t[1] and rc is t[2] and rw is t[4]
    # one cloud, one angle; no normals
    p1, _, _, n1, _ = pn2.random_rotate(t[0][1], None, None, None, None, alpha=alpha[1])
    assert n1 is None and torch.equal(p1, rp[1])
    # alpha from the generator: uniform in [0, 2 pi), reproducible
    a = pn2.random_rotate(t[0], None, None, None, None, generator=torch.Generator().manual_seed(4))
    b = pn2.random_rotate(t[0], None, None, None, None, generator=torch.Generator().manual_seed(4))
    assert torch.equal(a[0], b[0]) and not torch.equal(a[0], t[0])
    assert pn2.rotation_cs(0.0).tolist() == [1.0, 0.0] and pn2.rotation_cs([0.0, 1.0]).shape == (2, 2)
    # get_data_tensors: train.py:94-108 in one call
    for color, normal in ((True, True), (True, False), (False, True), (False, False)):
        xyz, labels, feats, smpw = pn2.get_data_tensors((pts, lab.astype(np.int64), col, nrm, sw),
                                                        color, normal, device="cpu")
        w = fc.feed_batch_numpy(pts, lab, col, nrm, sw, None, pn2.CLASS_WEIGHTS, color, normal)
        assert labels.dtype == torch.int32 and np.array_equal(labels.numpy(), lab)
        assert np.array_equal(fc.bits(xyz.numpy()), fc.bits(pts))
        assert np.array_equal(fc.bits(smpw.numpy()), fc.bits(w[2]))
        if color or normal:
            assert np.array_equal(fc.bits(feats.numpy()), fc.bits(w[1]))
        else:
            assert feats is None


# ------------------------------------------------------------------ class weights
def test_class_weights_are_the_formula_of_the_recorded_counts(pn2):
    counts = json.load(open(os.path.join(HERE, "golden", "class_counts.json")))["counts"]
    ccw = pn2.compute_class_weights
    w = ccw.weights_from_counts(counts)
    assert w.dtype == np.float64 and list(w[1:]) == pn2.CLASS_WEIGHTS[1:]
    assert pn2.CLASS_WEIGHTS[0] == 0 and pn2.CLASS_WEIGHTS == pn2.data_transformation.LABEL_WEIGHTS
    scenes = [np.array([1, 2, 2, 40, 39, 13, 14, 99, -3]), torch.tensor([16, 16, 0])]
    w2, cnt = ccw.get_weights(scenes)
    want = np.zeros(21, np.int64)
    for v in (1, 2, 2, 0, 20, 0, 13, 0, 0, 14, 14, 0):
        want[v] += 1
    assert cnt.tolist() == want.tolist() and np.array_equal(w2, ccw.weights_from_counts(want))


# ------------------------------------------------------------------ the epoch loop
class StubMetrics:
    def __init__(self, ious):
        self.ious, self.resets = list(ious), 0

    def iou(self):
        return torch.tensor(self.ious.pop(0)), None

    def reset(self):
        self.resets += 1


class StubOpt:
    def __init__(self):
        self.t = 0

    def state_dict(self):
        return {"global_step": np.int64(self.t)}


class StubStore(dict):
    def state_dict(self):
        return {"fc2/weights": np.ones(2, np.float32)}


def test_train_loop_epochs_validation_and_best_model(pn2, tmp_path):
    tr = pn2.train
    pts, lab, col, nrm, sw, _ = feed_inputs(2, 8)
    batch = (pts, lab, col, nrm, sw)
    seen = {"steps": [], "evals": 0, "models": set()}
    opt = StubOpt()

    def step_fn(store, o, metrics, xyz, labels, smpw, num_class, bn_decay=None,
                learning_rate=None, features=None, seed=None, model=None):
        assert features.shape == (2, 8, 6) and xyz.device.type == "cpu"
        seen["steps"].append((o.t, learning_rate, bn_decay, seed))
        seen["models"].add(model)
        o.t += 1
        return torch.tensor(float(o.t)), torch.tensor([1, 2])

    def eval_fn(store, metrics, xyz, labels, smpw, num_class, features=None, model=None):
        seen["evals"] += 1
        return torch.tensor(2.0), torch.tensor([3, 4])

    # bpe = 2.5: 15 steps; epochs end at steps 2, 4, ..., 14 with the reference's epoch numbers
    val_ious = [0.3, 0.2, 0.5]
    hist = tr.train(StubStore(), [batch], [batch, batch], epochs=6, batch_size=16,
                    n_train_samples=40, n_epochs_to_val=2, save_dir=str(tmp_path), step_fn=step_fn,
                    eval_fn=eval_fn, device="cpu", optimizer=opt, seed=100,
                    metrics=StubMetrics([0.1] * 7), val_metrics=StubMetrics(val_ious))
    assert len(seen["steps"]) == 15 and seen["models"] == {pn2.pointnet2_sem_seg.model_body}
    assert [s[0] for s in seen["steps"]] == list(range(15))
    assert [s[3] for s in seen["steps"]] == list(range(100, 115))
    assert seen["steps"][0][1:3] == (tr.get_learning_rate(0, 16, 40), tr.get_bn_decay(0, 16, 40))
    assert [h["step"] for h in hist] == [2, 4, 6, 8, 10, 12, 14]
    assert [h["epoch"] for h in hist] == [int(s / 2.5) + 1 for s in (2, 4, 6, 8, 10, 12, 14)] \
        == [1, 2, 3, 4, 5, 5, 6]
    # mean loss = the epoch's sum over bpe (train.py:209): steps (1,2) -> 3 / 2.5
    assert hist[0]["loss"] == 3 / 2.5 and hist[0]["accuracy"] == 1.0 / 2.5
    assert hist[0]["iou"] == pytest.approx(0.1)
    val = [h for h in hist if "val_iou" in h]
    assert [h["epoch"] for h in val] == [2, 4, 6] and seen["evals"] == 6
    assert [h["val_iou"] for h in val] == pytest.approx(val_ious)
    assert val[0]["val_loss"] == 2.0 and val[0]["val_accuracy"] == 0.75
    # saved only on improvement: 0.3 (> 0), not 0.2, then 0.5
    assert sorted(os.listdir(tmp_path)) == ["best_model_epoch_002.npz", "best_model_epoch_006.npz"]
    assert val[1]["saved"] is None and val[2]["saved"].endswith("best_model_epoch_006.npz")
    saved = np.load(val[2]["saved"])
    assert set(saved.files) == {"fc2/weights", "global_step"} and int(saved["global_step"]) == 14


def test_train_asserts_and_model_choice(pn2):
    tr = pn2.train
    for kw in (dict(use_color=True, use_normal=True, use_attention=True),
               dict(use_color=True, use_normal=False, use_attention=True),
               dict(use_color=False, use_normal=True, use_attention=True),
               dict(use_color=False, use_normal=False, use_attention=True, attention_single_layer=1)):
        with pytest.raises(AssertionError):
            tr.train(StubStore(), [], epochs=0, device="cpu", **kw)
    with pytest.raises(AssertionError):  # the reference's first assert: colour == attention
        tr.choose_model(False, False, False)
    body = pn2.pointnet2_sem_seg.model_body
    assert tr.choose_model(True, True) is body
    # the remaining branches need use_color != use_attention and use_normal != use_attention
    assert tr.choose_model(False, False, True) is pn2.pointnet2_sem_seg_attention.body
    sl = pn2.pointnet2_sem_seg_attention_single_layer
    with pytest.raises(AssertionError):
        sl.get_model(torch.zeros(1, 8, 3), 4, False, 21)
    with pytest.raises(AssertionError):
        sl.get_model(torch.zeros(1, 8, 3), -1, False, 21)
    att, pool = pn2.attention_layer.pointnet_sa_module_attention, \
        pn2.attention_layer.pointnet_sa_module_attention_and_pooling
    sa = pn2.pointnet_util.pointnet_sa_module
    assert sl.sa_modules(2) == (sa, sa, att, sa)
    assert pn2.pointnet2_sem_seg_attention.SA_MODULES == (att,) * 4
    assert pn2.pointnet2_sem_seg_attention_and_pooling.SA_MODULES == (pool,) * 4


# ------------------------------------------------------------------ the C ABI and the ops
def test_guards_return_einval_before_any_access(pn2):
    lib = pn2.lib()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big_s, big_n = 65535, 2 ** 31 // 65535 + 1          # S * N just past 2^31 - 1
    assert big_s * big_n > 2 ** 31 - 1
    for f, tail in ((lib.pn2_val_select, (p, 64, p, p, p, None)), (lib.pn2cpu_val_select, (p, p, p))):
        assert f(p, big_n, p, big_s, 0.2, 0.001, *tail) == E
        assert f(p, -1, p, 1, 0.2, 0.001, *tail) == E
        assert f(p, 1, p, 65536, 0.2, 0.001, *tail) == E
    assert lib.pn2_val_select(p, 4, p, 1, 0.2, 0.001, p, 64, None, p, p, None) == E   # counts NULL
    assert lib.pn2_val_select(p, 4, p, 1, 0.2, 0.001, p, 0, p, p, p, None) == E       # workspace
    assert lib.pn2cpu_val_select(p, 4, p, 1, 0.2, 0.001, p, None, p) == E

    def chunks(cpu, N=4, S=1, K=2, out=p, kept=p, choice=p, L=0):
        head = (p, p, None, None, N, p, p, p, S, choice, None, K, None, L, 0.01)
        if cpu:
            return lib.pn2cpu_val_chunks(*head, out, p, None, None, p, p, kept)
        return lib.pn2_val_chunks(*head, p, 64, out, p, None, None, p, p, kept, None)
    for cpu in (False, True):
        assert chunks(cpu, K=-1) == E                   # a negative npoints
        assert chunks(cpu, N=big_n, S=big_s) == E       # S * N past 2^31 - 1
        assert chunks(cpu, S=big_s, K=big_n) == E       # S * K past 2^31 - 1
        assert chunks(cpu, out=None) == E and chunks(cpu, kept=None) == E  # NULL outputs
        assert chunks(cpu, choice=None) == E            # neither choice nor u
        assert chunks(cpu, L=3) == E                    # L > 0 without the table

    def feed(cpu, B=1, N=2, xyz=p, smpw=p, feats=None, uc=0, un=0, colors=None, L=0):
        args = (p, p, colors, None, p, None, None, L, B, N, uc, un, xyz, feats, smpw)
        return lib.pn2cpu_feed_batch(*args) if cpu else lib.pn2_feed_batch(*args, None)
    for cpu in (False, True):
        assert feed(cpu, B=-1) == E and feed(cpu, N=-1) == E and feed(cpu, L=-1) == E
        assert feed(cpu, xyz=None) == E and feed(cpu, smpw=None) == E     # NULL outputs
        assert feed(cpu, uc=1) == E and feed(cpu, un=1) == E              # flags without inputs
        assert feed(cpu, uc=1, colors=p) == E                             # F > 0, features NULL
        assert feed(cpu, L=21) == E
        assert feed(cpu, B=0) == 0
    assert lib.pn2_val_select_workspace_size(4097, 3) == 3 * 2 * 4
    assert lib.pn2_val_chunks_workspace_size(20) == 80


def test_schemas_kernels_and_exports(pn2, ops):
    assert ops.FEED_NAMES == ("feed_batch", "val_select", "val_chunks")
    for name in ops.FEED_NAMES:
        assert name in ops.__all__
        for key in ("CUDA", "Meta", "CPU"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key), (name, key)
    assert str(ops.val_select._schemas[""]) == \
        "pn2::val_select(Tensor points, Tensor bounds, float margin, float inner_margin) -> " \
        "(Tensor counts, Tensor sel, Tensor inner)"
    for name in ("pointnet2_sem_seg_attention", "pointnet2_sem_seg_attention_and_pooling",
                 "pointnet2_sem_seg_attention_single_layer", "compute_class_weights", "random_rotate",
                 "scene_val_chunks", "get_data_tensors", "eval_model", "CLASS_WEIGHTS"):
        assert name in pn2.__all__ and hasattr(pn2, name), name
    import pn2hip
    assert pn2hip.train.train is pn2.train.train and pn2hip.get_data_tensors is pn2.get_data_tensors
    assert not hasattr(pn2.data_transformation, "get_all_subsets_for_scene")


def test_meta_shapes_and_checks(ops):
    m = lambda *s, dt=torch.float32: torch.empty(s, device="meta", dtype=dt)  # noqa: E731
    i = lambda *s: m(*s, dt=torch.int32)  # noqa: E731
    xyz, f, w = ops.feed_batch(m(2, 9, 3), i(2, 9), i(2, 9, 3), m(2, 9, 3), m(2, 9), m(2, 2), m(21),
                               True, True)
    assert (xyz.shape, f.shape, w.shape) == ((2, 9, 3), (2, 9, 6), (2, 9))
    assert ops.feed_batch(m(2, 9, 3), i(2, 9), None, None, m(2, 9), None, m(21), False,
                          False)[1].shape == (2, 9, 0)
    c, s, n = ops.val_select(m(50, 3), m(4, 6, dt=torch.float64), 0.2, 0.001)
    assert (c.shape, s.shape, n.shape, n.dtype) == ((4,), (4, 50), (4, 50), torch.uint8)
    out = ops.val_chunks(m(50, 3), i(50), i(50, 3), None, c, s, n, i(4, 16), None, 16, m(21), 0.01)
    assert [tuple(t.shape) for t in out] == [(4, 16, 3), (4, 16), (4, 16, 3), (0,), (4, 16), (4,),
                                             (1,)]
    bad = [
        lambda: ops.feed_batch(m(2, 9, 3), i(2, 9), None, None, m(2, 9), None, m(21), True, False),
        lambda: ops.feed_batch(m(2, 9, 3), i(2, 8), None, None, m(2, 9), None, m(21), False, False),
        lambda: ops.feed_batch(m(2, 9, 3), i(2, 9), None, None, m(2, 9), m(3, 2), m(21), False, False),
        lambda: ops.feed_batch(m(2, 9, 3), m(2, 9), None, None, m(2, 9), None, m(21), False, False),
        lambda: ops.val_select(m(50, 3), m(4, 6), 0.2, 0.001),
        lambda: ops.val_select(m(2 ** 20, 3), m(4096, 6, dt=torch.float64), 0.2, 0.001),
        lambda: ops.val_chunks(m(50, 3), i(50), None, None, c, s, n, None, None, 16, m(21), 0.01),
        lambda: ops.val_chunks(m(50, 3), i(50), None, None, c, s, n, i(4, 15), None, 16, m(21), 0.01),
        lambda: ops.val_chunks(m(50, 3), i(50), None, None, c, s, n, None, m(4, 16), -1, m(21), 0.01),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
