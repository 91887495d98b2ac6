"""MI355X: every torch.ops.pn2 operator under the Meta key against the same call on the device.
One body serves both keys (csrc/torch_ops.cpp) and returns for Meta after its allocations, so for
one small valid call per op, and for the empty inputs whose early returns sit beside the Meta
one, every output has the device output's shape, dtype and stride, and the ops that write in
place return the same structure. Nothing here depends on a workload size: the shapes are the
smallest at which each op is defined."""
import pytest

pytestmark = pytest.mark.gpu

B, N, M, NS, C, COUT, NCLS, SCENE = 2, 40, 8, 4, 8, 16, 21, 50  # C % 4 == 0 (key_dim 4)

OPS = ("farthest_point_sample", "farthest_point_sample_and_gather", "gather_point",
       "gather_point_grad", "prob_sample", "query_ball_point", "select_top_k", "knn_point",
       "group_point", "group_point_grad", "group_concat", "three_nn", "three_interpolate",
       "three_interpolate_grad", "idw_weights", "fp_fused", "attn_reduce", "attn_reduce_grad",
       "group_pool", "mlp_layer_train", "mlp_layer_train_grad", "mlp_layer_train_pool",
       "mlp_layer_train_pool_grad", "attn_kv_train", "attn_kv_train_grad", "bn_train",
       "bn_train_grad", "dropout", "softmax_xent", "softmax_xent_grad", "group_concat_train",
       "group_concat_train_grad", "fp_apply_train", "fp_apply_train_grad", "adam_step",
       "seg_confusion", "mean_iou", "scene_vote", "scene_labels", "map_back_rows", "label_lut")
# B = 0, zero rows, zero groups
EMPTY = ("farthest_point_sample_and_gather", "mlp_layer_train", "bn_train", "softmax_xent",
         "attn_kv_train_grad")
IN_PLACE = ("adam_step", "seg_confusion", "scene_vote", "map_back_rows")
CASES = OPS + tuple(name + "-empty" for name in EMPTY)


@pytest.fixture(scope="module")
def env():
    import torch

    import pn2hip
    return pn2hip.ops, torch


def _table(torch, dev):
    """case -> the arguments of one valid call, on the device (every index in range)."""
    gen = torch.Generator().manual_seed(0)
    f = lambda *s: torch.rand(s, generator=gen).to(dev)  # noqa: E731
    i = lambda hi, *s: torch.randint(0, hi, s, generator=gen, dtype=torch.int32).to(dev)  # noqa: E731
    z64 = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)  # noqa: E731
    xyz, new_xyz, pts, pts2 = f(B, N, 3), f(B, M, 3), f(B, N, C), f(B, M, C)
    idx2, idx3, nn3 = i(N, B, M), i(N, B, M, NS), i(M, B, N, 3)
    x, w, b = f(B, M, NS, C), f(C, COUT), f(COUT)
    y, arg = f(B, M, NS, COUT), i(NS, B, M, COUT)
    wc, bc = f(C, C), f(C)
    Q, K = f(B, M, C), f(B, M, NS, C)
    logits, labels, wts = f(B, N, NCLS), i(NCLS, B, N), f(B, N)
    adam = [[f(3, 4), f(7)] for _ in range(4)]
    keys, lut = z64(SCENE), torch.arange(NCLS, dtype=torch.int32, device=dev)
    t = {
        "farthest_point_sample": (M, xyz),
        "farthest_point_sample_and_gather": (M, xyz),
        "farthest_point_sample_and_gather-empty": (M, f(0, N, 3)),
        "gather_point": (xyz, idx2),
        "gather_point_grad": (xyz, idx2, f(B, M, 3)),
        "prob_sample": (f(B, N), f(B, M)),
        "query_ball_point": (0.5, NS, xyz, new_xyz),
        "select_top_k": (3, f(B, M, N)),
        "knn_point": (3, xyz, new_xyz),
        "group_point": (pts, idx3),
        "group_point_grad": (pts, idx3, f(B, M, NS, C)),
        "group_concat": (xyz, pts, new_xyz, idx3, True, False),
        "three_nn": (xyz, new_xyz),
        "three_interpolate": (pts2, nn3, f(B, N, 3)),
        "three_interpolate_grad": (pts2, nn3, f(B, N, 3), f(B, N, C)),
        "idw_weights": (f(B, N, 3),),
        "fp_fused": (xyz, new_xyz, pts, pts2),
        "attn_reduce": (Q, K, f(B, M, NS, C)),
        "attn_reduce_grad": (Q, K, f(B, M, NS, C), f(B, M, C)),
        "group_pool": (K, None, 3),
        "mlp_layer_train": (x, w, b, f(COUT), f(COUT), 1e-3, True),
        "mlp_layer_train-empty": (f(0, C), w, b, f(COUT), f(COUT), 1e-3, True),
        "mlp_layer_train_grad": (f(B, M, NS, COUT), x, w, y, f(COUT), f(COUT), f(COUT), f(COUT),
                                 1e-3, True, True),
        "mlp_layer_train_pool": (x, w, b, f(COUT), f(COUT), 1e-3, True),
        "mlp_layer_train_pool_grad": (f(B, M, COUT), arg, x, w, y, f(COUT), f(COUT), f(COUT),
                                      f(COUT), 1e-3, True, True),
        "attn_kv_train": (x, wc, bc, wc, bc, wc, bc, True),
        "attn_kv_train_grad": (f(B, M, C), f(B, M, C), i(NS, B, M, C), x, wc, wc, wc, f(B, M, C),
                               f(B, M, NS, 2 * C), True),
        "attn_kv_train_grad-empty": (f(0, C), None, i(1, 0), f(0, NS, C), wc, wc, wc, f(0, C),
                                     f(0, NS, 2 * C), True),
        "bn_train": (Q, bc, bc, 1e-3, False),
        "bn_train-empty": (f(0, C), bc, bc, 1e-3, False),
        "bn_train_grad": (f(B, M, C), Q, bc, bc, bc, bc, 1e-3, False),
        "dropout": (pts, 0.5, 7),
        "softmax_xent": (logits, labels, wts),
        "softmax_xent-empty": (f(0, NCLS), i(NCLS, 0), None),
        "softmax_xent_grad": (f(), logits, labels, wts, f(B, N),
                              torch.tensor(B * N, dtype=torch.int32, device=dev)),
        "group_concat_train": (xyz, pts, new_xyz, idx3, True, False),
        "group_concat_train_grad": (f(B, M, NS, C + 3), idx3, N, C, 3),
        "fp_apply_train": (f(B, N, 3), nn3, pts, pts2),
        "fp_apply_train_grad": (f(B, N, 2 * C), f(B, N, 3), nn3, M, C, C),
        "adam_step": (*adam, 1e-3, 0.9, 0.999, 1e-8),
        "seg_confusion": (labels, i(NCLS, B, N), z64(NCLS, NCLS), z64(2)),
        "mean_iou": (z64(NCLS, NCLS) + 1,),
        "scene_vote": (f(SCENE, NCLS), torch.ones(SCENE, dtype=torch.uint8, device=dev),
                       i(SCENE, SCENE), 0, keys),
        "scene_labels": (z64(SCENE), lut, 0),
        "map_back_rows": (f(SCENE, 3), 0, z64(SCENE), f(SCENE, 3)),
        "label_lut": (i(NCLS + 4, SCENE), lut, -1),
    }
    return t


@pytest.fixture(scope="module")
def table(env):
    return _table(env[1], env[1].device("cuda:0"))


def _to_meta(torch, a):
    if isinstance(a, torch.Tensor):
        return a.to("meta")
    if isinstance(a, list):
        return [_to_meta(torch, v) for v in a]
    return a


def _outputs(torch, out):
    if out is None:
        return ()
    return (out,) if isinstance(out, torch.Tensor) else tuple(out)


@pytest.mark.parametrize("case", CASES)
def test_meta_agrees_with_the_device(env, table, case):
    ops, torch = env
    op = getattr(ops, case.split("-")[0])
    args = table[case]
    meta_args = tuple(_to_meta(torch, a) for a in args)
    got, want = op(*meta_args), op(*args)
    torch.cuda.synchronize()
    assert type(got) is type(want), (type(got), type(want))
    if case in IN_PLACE:  # nothing comes back but scene_vote's pred, next to the keys it writes
        assert (got is None) == (case != "scene_vote")
    got, want = _outputs(torch, got), _outputs(torch, want)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.is_meta and w.is_cuda, k
        assert (g.shape, g.dtype, g.stride()) == (w.shape, w.dtype, w.stride()), k


def test_every_op_has_a_row(env, table):
    ops, _ = env
    assert set(OPS) == set(ops.NAMES + ops.HOST_NAMES)
    assert set(table) == set(CASES) and set(IN_PLACE) <= set(OPS)
