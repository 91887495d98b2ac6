"""GPU: whole-scene prediction on the device (csrc/predict.hip) against its host twins
(csrc/cpu_predict.cpp, the CPU kernels of the same torch ops) and against the reference's numpy
route (np.argmax + map_back, generate_predictions.py:19-37, :139-186). Everything is integers
and copied bytes: every comparison is exact.

The kernel cases cover a partial wave (1, 63 rows), the wave edges (64, 65), more than one
workgroup (2049), more rows than one workgroup's share of a chunk batch (3 x 8192 + 5) and one
row count past the grid (2048 workgroups x 256 rows), where rows are grid-strided; C = 1, 2 (even,
the padded LDS stride), 21 (one tile), 22 and 256 (column tiles, the last one partial / full).

predict_scene runs on golden scene 1 (20 000 points, np.random.seed(7)), which the chunker cuts
into 20 chunks. Two things about that scene are not as the issue that asked for this test
assumed, and the test asks for them in another way:
- 20 chunks give no smaller final batch at batch = 2, so the scene also runs at batch = 3 (six
  batches of 3 and one of 2);
- none of its points lies on a column boundary (the boundaries are min + 1.5 i in float64, the
  coordinates random float32: every point is written exactly once), so the tie rule is not
  exercised there. The "boundary" scene is the same scene moved so that its lowest x and y are
  exactly 0, with 60 points put on x = 1.5, 30 of them also on y = 1.5: those lie in two or
  four inner boxes, are written two or four times, and the test asserts it."""
import importlib
import os

import numpy as np
import pytest

from conftest import PKG_NAME
from support import gpu_marks

pytestmark = gpu_marks


@pytest.fixture(scope="module")
def env():
    import torch

    import pn2hip
    pkg = importlib.import_module(PKG_NAME)
    return pkg, pn2hip.ops, torch, torch.device("cuda:0")


def numpy_map_back(values, original_idx, mask, res_shape):
    """generate_predictions.py:19-37."""
    values = values[mask]
    original_idx = original_idx[mask]
    res = np.zeros(res_shape)
    res[original_idx] = values
    return res


def _rows(rng, rows, C, n):
    """Logits drawn from 8 values (ties are frequent), a 60 % mask, indices partly outside."""
    logits = None if C is None else rng.randint(0, 8, (rows, C)).astype(np.float32)
    mask = rng.uniform(size=rows) < 0.6
    orig = rng.randint(-1, n + 1, rows).astype(np.int32)
    return logits, mask, orig


def _run(ops, torch, dev, logits, mask, orig, row0, n, values):
    """vote + labels + map_back_rows on `dev`; everything back on the host as numpy."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    pred = ops.scene_vote(t(logits), t(mask), t(orig), row0, keys)
    lut = torch.arange(300, 300 + 200, dtype=torch.int32, device=dev)
    labels, mapped, winner = ops.scene_labels(keys, lut, -5)
    outs = []
    for v in values:
        out = torch.full((n,) + v.shape[1:], 7, dtype=torch.float32, device=dev)
        ops.map_back_rows(t(v), row0, keys, out)
        outs.append(out)
    return [x.cpu().numpy() for x in [keys, pred, labels, mapped, winner] + outs]


@pytest.mark.parametrize("C", [1, 2, 21, 22, 256])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 2049, 3 * 8192 + 5])
def test_kernels_equal_the_twins(env, rows, C):
    pkg, ops, torch, dev = env
    rng = np.random.RandomState(rows % 1000 + C)
    n = max(1, rows // 3)
    logits, mask, orig = _rows(rng, rows, C, n)
    values = [rng.uniform(-1, 1, (rows,) + tail).astype(np.float32) for tail in ((), (3,), (4,), (21,))]
    row0 = 5 * 8192
    want = _run(ops, torch, "cpu", logits, mask, orig, row0, n, values)
    got = _run(ops, torch, dev, logits, mask, orig, row0, n, values)
    again = _run(ops, torch, dev, logits, mask, orig, row0, n, values)
    names = ["keys", "pred_rows", "labels", "mapped", "winner", "out4", "out12", "out16", "out84"]
    for name, w, g, a in zip(names, want, got, again):
        assert w.dtype == g.dtype and np.array_equal(w.view(np.uint8), g.view(np.uint8)), name
        assert np.array_equal(g.view(np.uint8), a.view(np.uint8)), name  # two runs, equal bits
    assert np.array_equal(got[1], np.argmax(logits, axis=1))


@pytest.mark.parametrize("C", [None, 2])
def test_rows_past_the_grid_are_strided(env, C):
    """2048 workgroups of 256 rows is the largest grid: the rows after it take a second pass."""
    pkg, ops, torch, dev = env
    rows, n = 2048 * 256 + 65, 1000
    rng = np.random.RandomState(11)
    logits, mask, orig = _rows(rng, rows, C, n)
    want = _run(ops, torch, "cpu", logits, mask, orig, 0, n, [])
    got = _run(ops, torch, dev, logits, mask, orig, 0, n, [])
    for w, g in zip(want, got):
        assert np.array_equal(w, g)
    assert got[4].max() >= 2048 * 256  # a row of the second pass won somewhere


@pytest.mark.parametrize("rows,n", [(8192, 1), (65536, 17)])
def test_contention(env, rows, n):
    """Every row of a chunk votes for one point; 65 536 rows vote over 17 points."""
    pkg, ops, torch, dev = env
    rng = np.random.RandomState(rows)
    logits = rng.randint(0, 8, (rows, 21)).astype(np.float32)
    mask = np.ones(rows, bool)
    orig = rng.randint(0, n, rows).astype(np.int32)
    want = _run(ops, torch, "cpu", logits, mask, orig, 0, n, [])
    for _ in range(2):
        got = _run(ops, torch, dev, logits, mask, orig, 0, n, [])
        for w, g in zip(want, got):
            assert np.array_equal(w, g)
    last = np.array([np.flatnonzero(orig == q).max() for q in range(n)])
    assert np.array_equal(got[4], last)  # numpy's last write wins
    assert np.array_equal(got[2], np.argmax(logits, axis=1)[last])


def test_batch_order_and_streams_do_not_matter(env):
    pkg, ops, torch, dev = env
    rng = np.random.RandomState(5)
    rows, n = 5 * 4096 + 77, 900
    logits, mask, orig = _rows(rng, rows, 21, n)
    cuts = [0, 4096, 4097, 9000, 16384, rows]
    L, M, O = (torch.from_numpy(a).to(dev) for a in (logits, mask, orig))
    one = torch.zeros(n, dtype=torch.int64, device=dev)
    ops.scene_vote(L, M, O, 0, one)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    for order in (range(5), reversed(range(5))):
        keys = torch.zeros(n, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        for b in order:
            a, z = cuts[b], cuts[b + 1]
            with torch.cuda.stream(streams[b % 2]):
                ops.scene_vote(L[a:z], M[a:z], O[a:z], a, keys)
        torch.cuda.synchronize(dev)
        assert torch.equal(keys, one)


def test_map_back_rows_batch_by_batch(env):
    pkg, ops, torch, dev = env
    rng = np.random.RandomState(9)
    rows, n = 3 * 8192, 7000
    _, mask, orig = _rows(rng, rows, None, n)
    values = torch.from_numpy(rng.uniform(-1, 1, (rows, 3)).astype(np.float32)).to(dev)
    keys = torch.zeros(n, dtype=torch.int64, device=dev)
    ops.scene_vote(None, torch.from_numpy(mask).to(dev), torch.from_numpy(orig).to(dev), 0, keys)
    whole = torch.full((n, 3), 5.0, device=dev)
    ops.map_back_rows(values, 0, keys, whole)
    parts = torch.full((n, 3), 5.0, device=dev)
    winner = ops.scene_labels(keys, None, 0)[2]
    for a in (8192, 0, 16384):  # any order
        before = parts.clone()
        ops.map_back_rows(values[a:a + 8192], a, keys, parts)
        outside = (winner >= 0) & ((winner < a) | (winner >= a + 8192))
        assert outside.any() and torch.equal(parts[outside], before[outside])  # left untouched
    assert torch.equal(whole, parts)
    ok = mask & (orig >= 0) & (orig < n)
    assert np.array_equal(whole.cpu().numpy(), numpy_map_back(values.cpu().numpy(), orig, ok, (n, 3)))
    assert (winner < 0).any() and not whole[winner < 0].any()  # unwritten points: zero bytes


# ------------------------------------------------------------------ predict_scene
@pytest.fixture(scope="module")
def scene(env):
    pkg = env[0]
    return pkg.synth.scannet_scene(1, 20000)


def _model(pkg, store, with_feats):
    if with_feats:
        return lambda xyz, feats: pkg.pointnet2_sem_seg_features.get_model(
            xyz, feats, False, 21, params=store)[0]
    return lambda xyz, feats: pkg.pointnet2_sem_seg.get_model(xyz, False, 21, params=store)[0]


def _boundary_scene(scene):
    pts, lab, col, nrm = scene
    pts = pts.copy()
    pts[:, 0] -= pts[:, 0].min()
    pts[:, 1] -= pts[:, 1].min()
    assert pts[:, 0].min() == 0 and pts[:, 1].min() == 0 and pts[:, 0].max() > 3
    pick = np.random.RandomState(1).choice(len(pts), 60, replace=False)
    pts[pick, 0] = 1.5
    pts[pick[:30], 1] = 1.5
    return pts, lab, col, nrm


@pytest.mark.parametrize("kind,with_feats,with_labels,batch", [
    ("golden", False, True, 2), ("golden", True, True, 2), ("golden", True, False, 3),
    ("boundary", True, True, None)])
def test_predict_scene_equals_the_numpy_route(env, scene, kind, with_feats, with_labels, batch):
    pkg, ops, torch, dev = env
    pts, lab, col, nrm = scene if kind == "golden" else _boundary_scene(scene)
    N = len(pts)
    store = pkg.tf_util.ParamStore(seed=3)
    model = _model(pkg, store, with_feats)
    # by hand: the same chunks and batches through the same model call, then the reference's
    # host route
    csl = pkg.complete_scene_loader
    zc, zn = np.zeros((N, 3), np.int32), np.zeros((N, 3), np.float32)
    np.random.seed(7)
    if with_labels:
        P, Lb, Cc, Nn, _, masks, orig = csl.get_all_subsets_with_all_points_for_scene_numpy(
            pts, lab, col if with_feats else zc, nrm if with_feats else zn)
    else:
        P, Cc, Nn, masks, orig = csl.get_all_subsets_with_all_points_for_scene_numpy_test(
            pts, col if with_feats else zc, nrm if with_feats else zn)
    X = P.shape[0]
    if kind == "golden":
        assert X == 20
    else:
        batch = next(b for b in (3, 4, 5, 7) if X % b)  # a final smaller batch
    np.random.seed(7)
    res = pkg.generate_predictions.predict_scene(
        model, pts, col if with_feats else None, nrm if with_feats else None,
        lab if with_labels else None, batch=batch, device=dev)
    sizes = []
    all_pred = []
    for b0 in range(0, X, batch):
        xyz = torch.from_numpy(P[b0:b0 + batch]).to(dev)
        feats = None
        if with_feats:
            c = torch.from_numpy(Cc[b0:b0 + batch]).to(dev).to(torch.float32) / 255.0
            feats = torch.cat([c, torch.from_numpy(Nn[b0:b0 + batch]).to(dev)], dim=2)
        logits = model(xyz, feats).cpu().numpy()
        sizes.append(logits.shape[0])
        all_pred.append(np.argmax(logits.reshape(-1, 21), axis=1))
    assert (sizes[-1] < batch) == (batch != 2)  # the final smaller batch
    all_pred = np.concatenate(all_pred)
    all_masks = np.array(masks.reshape(-1), dtype=bool)
    all_orig = orig.reshape(-1)
    writes = np.bincount(all_orig[all_masks], minlength=N)
    if kind == "boundary":  # points on a column boundary are written twice, on a corner 4 times
        assert (writes == 2).sum() >= 30 and (writes == 4).sum() >= 1
    assert len(np.unique(all_pred)) > 1
    want_pred = numpy_map_back(all_pred, all_orig, all_masks, N)
    want_points = numpy_map_back(P.reshape(-1, 3), all_orig, all_masks, (N, 3))
    assert np.array_equal(res["labels"].cpu().numpy(), want_pred)
    assert res["labels"].dtype == torch.int32
    assert np.array_equal(res["points"].cpu().numpy(), want_points)
    nyu40 = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 10, 11: 11, 12: 12, 13: 14,
             14: 16, 15: 24, 16: 28, 17: 33, 18: 34, 19: 36, 20: 39}
    assert np.array_equal(res["nyu40"].cpu().numpy(), [nyu40.get(int(v), 1) for v in want_pred])
    if with_labels:
        want_gt = numpy_map_back(Lb.reshape(-1), all_orig, all_masks, N)
        assert np.array_equal(res["gt_labels"].cpu().numpy(), want_gt)
    else:
        assert "gt_labels" not in res
    winner = res["winner"].cpu().numpy()
    assert np.array_equal(res["points"].cpu().numpy()[winner >= 0], pts[winner >= 0])
    assert np.array_equal(winner >= 0, np.bincount(all_orig[all_masks], minlength=N) > 0)


def test_generate_predictions_then_evaluate(env, scene, tmp_path):
    pkg, ops, torch, dev = env
    gp, ev = pkg.generate_predictions, pkg.evaluate
    pts, lab, col, nrm = scene
    store = pkg.tf_util.ParamStore(seed=3)
    model = _model(pkg, store, True)
    np.random.seed(7)
    names = gp.generate_predictions(model, [("scene0001_00", pts, col, nrm, lab)], str(tmp_path),
                                    batch=8, device=dev)
    assert names == ["scene0001_00"]
    labels = np.load(tmp_path / "labels" / "scene0001_00.npy")
    gt = np.load(tmp_path / "groundtruth_labels" / "scene0001_00.npy")
    points = np.load(tmp_path / "points" / "scene0001_00.npy")
    assert labels.dtype == gt.dtype == points.dtype == np.float64  # map_back's arrays
    assert labels.shape == gt.shape == (len(pts),) and points.shape == (len(pts), 3)
    pred_file = str(tmp_path / "predictions" / "scene0001_00.txt")
    pred_ids = ev.load_ids(pred_file)
    assert np.array_equal(pred_ids, gp.map_to_nyu40(labels))
    # the ground truth in the benchmark's format: NYU-40 ids, 0 = unannotated
    gt_ids = np.where(gt > 0, gp.map_to_nyu40(gt), 0).astype(np.int64)
    gt_file = str(tmp_path / "gt.txt")
    gp.export_ids(gt_file, gt_ids)
    confusion, ious = ev.evaluate([pred_file], [gt_file], str(tmp_path / "result.txt"), device=dev)
    # evaluate.py:78-83, directly from the arrays
    want = np.zeros((41, 41), np.int64)
    valid = np.isin(gt_ids, ev.VALID_CLASS_IDS)
    col_ids = np.where(np.isin(pred_ids, ev.VALID_CLASS_IDS), pred_ids, 40)
    np.add.at(want, (gt_ids[valid], col_ids[valid]), 1)
    assert want.sum() > 10000
    assert np.array_equal(confusion.cpu().numpy(), want)
    assert ious["wall"] == ev.get_iou(1, want)
    assert os.path.getsize(tmp_path / "result.txt") > 0


def test_eval_step(env):
    pkg, ops, torch, dev = env
    xyz_np, feats_np = pkg.synth.batch([0, 1], 2048, "scannet", with_features=True)
    xyz, feats = torch.from_numpy(xyz_np).to(dev), torch.from_numpy(feats_np).to(dev)
    g = np.random.RandomState(2)
    labels = torch.from_numpy(g.randint(0, 21, (2, 2048)).astype(np.int32)).to(dev)
    smpw = torch.from_numpy(g.uniform(0.5, 5, (2, 2048)).astype(np.float32)).to(dev) * (labels > 0)
    store = pkg.tf_util.ParamStore(seed=4).trainable(dev)
    # one training step first: every variable exists and the moving statistics have moved
    opt, metrics = pkg.AdamOptimizer(store), pkg.SegMetrics(21, dev)
    pkg.train_step(store, opt, metrics, xyz, labels, smpw, 21, bn_decay=0.5, features=feats, seed=1)
    before = {k: v.detach().clone() for k, v in store.items()}
    metrics = pkg.SegMetrics(21, dev)
    loss, counts = pkg.eval_step(store, metrics, xyz, labels, smpw, 21, features=feats)
    assert not loss.requires_grad
    # by hand: the inference logits, the loss op, the confusion op
    with torch.no_grad():
        logits, _ = pkg.pointnet2_sem_seg_features.get_model(xyz, feats, False, 21, params=store)
        want_loss, _, pred, _ = ops.softmax_xent(logits, labels, smpw)
    cm = torch.zeros(21, 21, dtype=torch.int64, device=dev)
    want_counts = torch.zeros(2, dtype=torch.int64, device=dev)
    ops.seg_confusion(labels, pred, cm, want_counts)
    assert torch.equal(loss.view(torch.int32), want_loss.view(torch.int32))
    assert torch.equal(counts, want_counts) and int(counts[1]) == int((labels > 0).sum())
    assert torch.equal(metrics.confusion, cm)
    assert set(store) == set(before)
    for k, v in store.items():
        assert torch.equal(v.detach().view(torch.int32), before[k].view(torch.int32)), k
    # (the training step above did move the statistics that eval_step must leave alone)
    assert any(k.endswith("moving_mean") and bool(v.abs().sum() > 0) for k, v in store.items())
