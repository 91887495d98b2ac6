"""MI355X: scene rendering (csrc/render.hip; torch.ops.pn2.render_ball / render_project,
show3d_balls.py, visualization.py) against the reference's own images (tests/golden/
make_golden_render.py), the host twins (csrc/cpu_render.cpp) and the numpy restatement of the
key-max rule (tests/render_ref.py). Integers in, bytes out: every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

import render_ref
from support import gpu_marks

pytestmark = gpu_marks

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "render")
CALLS = render_ref.golden_calls(GOLDEN)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


@pytest.fixture(scope="module")
def palette():
    with open(os.path.join(GOLDEN, "palette.json")) as f:
        return np.array(json.load(f)["label_colors"], np.float32)


def t(a, dev=DEV):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ball(ops, ixyz, c, r, h, w, background, dev=DEV):
    """render_ball on `dev` for ixyz (F,n,3) or (n,3) and channels c (3,n): (F,h,w,3) numpy."""
    ixyz = np.asarray(ixyz, np.int32)
    ixyz = ixyz[None] if ixyz.ndim == 2 else ixyz
    out = ops.render_ball(t(ixyz, dev), t(c[0], dev), t(c[1], dev), t(c[2], dev), None, None,
                          int(r), int(h), int(w), [int(b) for b in background])
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CALLS))
def test_device_reproduces_the_reference_and_the_twin(ops, name):
    c = CALLS[name]
    args = (c["ixyz"], c["c"], c["r"], c["h"], c["w"], c["background"])
    got = ball(ops, *args)
    assert np.array_equal(got[0], c["image"]), f"{(got[0] != c['image']).sum()} bytes differ"
    assert np.array_equal(got, ball(ops, *args, dev="cpu"))
    assert np.array_equal(got, ball(ops, *args)), "two runs differ"


@pytest.mark.parametrize("name", ["viewer_f32", "viewer_f64"])
def test_projection_and_showpoints_reproduce_the_viewer(pn2, ops, name):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    s = pn2.show3d_balls
    xyz = s.prepare(g["points"], int(g["showsz"]))
    mats = s.view_matrices(float(g["xangle"]), float(g["yangle"]), float(g["zoom"]), 96, 96)
    got = ops.render_project(t(xyz), t(mats))
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy()[0], g["ixyz"])
    assert np.array_equal(ops.render_project(t(xyz, "cpu"), t(mats, "cpu")).numpy()[0], g["ixyz"])
    img = s.showpoints(t(g["points"]), t(g["colours"]), None,
                       background=tuple(int(b) for b in g["background"]),
                       normalizecolor=bool(g["normalizecolor"]), ballradius=int(g["ballradius"]),
                       xangle=float(g["xangle"]), yangle=float(g["yangle"]), zoom=float(g["zoom"]),
                       showsz=int(g["showsz"]))
    assert img.device.type == "cuda" and np.array_equal(img.cpu().numpy(), g["image"])


def test_frames_in_one_call_and_strided_inputs(ops):
    c = CALLS["direct_r4"]
    rng = np.random.RandomState(3)
    ixyz = c["ixyz"][None] + rng.randint(-6, 7, (3, 1, 3)).astype(np.int32)
    args = (c["c"], 4, c["h"], c["w"], c["background"])
    got = ball(ops, ixyz, *args)
    for f in range(3):
        assert np.array_equal(got[f], ball(ops, ixyz[f], *args)[0]), f
    assert np.array_equal(got, ball(ops, ixyz, *args, dev="cpu"))
    # strided and offset inputs give the contiguous result
    wide = torch.zeros(3, len(c["ixyz"]), 5, dtype=torch.int32, device=DEV)
    wide[:, :, 1:4] = t(ixyz)
    cols = t(c["c"].T)  # (n, 3): each channel has stride 3, two of them start off 16 bytes
    bg = [int(b) for b in c["background"]]
    got2 = ops.render_ball(wide[:, :, 1:4], cols[:, 0], cols[:, 1], cols[:, 2], None, None, 4,
                           c["h"], c["w"], bg)
    assert np.array_equal(got2.cpu().numpy(), got)
    xyz = rng.randn(301, 3) * 30
    mats = rng.randn(2, 12)
    want = np.stack([render_ref.project(xyz, m) for m in mats])
    xw = torch.zeros(301, 7, dtype=torch.float64, device=DEV)
    xw[:, 2:5] = t(xyz)
    mw = torch.zeros(2, 14, dtype=torch.float64, device=DEV)
    mw[:, 1:13] = t(mats)
    assert np.array_equal(ops.render_project(xw[:, 2:5], mw[:, 1:13]).cpu().numpy(), want)
    assert np.array_equal(ops.render_project(t(xyz), t(mats)).cpu().numpy(), want)
    x32 = xyz.astype(np.float32)
    want32 = np.stack([render_ref.project(x32, m) for m in mats])
    assert np.array_equal(ops.render_project(t(x32)[1:], t(mats)).cpu().numpy(), want32[:, 1:])


def test_many_contenders_per_pixel_keep_the_index_high_bits(ops):
    """70,001 points on a 64 x 64 image at radius 1: about 17 points per pixel and only 5 depths,
    so most pixels are decided among equal z2 by the point index, past 65,536 too."""
    rng = np.random.RandomState(6)
    n, h, w = 70001, 64, 64
    ixyz = np.stack([rng.randint(-2, h + 2, n), rng.randint(-2, w + 2, n), rng.randint(0, 5, n)], 1)
    ixyz = ixyz.astype(np.int32)
    ixyz[:66000, 2] = 0  # the deepest points all come after index 65,536 on many pixels
    c = rng.uniform(0, 255, (3, n)).astype(np.float32)
    keys = render_ref.keys_of(ixyz, 1, h, w)
    winners = 0xFFFFFFFF - (keys[keys != 0] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (winners > 65536).sum() > 1000 and (winners < 65536).sum() > 10
    want = render_ref.render_ball(ixyz, *c, 1, h, w, (5, 6, 7))
    assert np.array_equal(ball(ops, ixyz, c, 1, h, w, (5, 6, 7))[0], want)
    assert np.array_equal(ball(ops, ixyz, c, 0, h, w, (5, 6, 7), dev="cpu")[0], want)


def test_more_pixels_and_points_than_one_launch_covers(ops):
    """An image of more pixels than the resolve grid's threads (4096 x 256) and more points than
    the splat grid's waves (2048 x 4) take at once: both kernels run their grid-stride loops."""
    rng = np.random.RandomState(7)
    n, h, w, r = 9000, 1100, 1000, 3
    ixyz = np.stack([rng.randint(-3, h + 3, n), rng.randint(-3, w + 3, n),
                     rng.randint(-40, 40, n)], 1).astype(np.int32)
    c = rng.uniform(0, 255, (3, n)).astype(np.float32)
    got = ball(ops, ixyz, c, r, h, w, (0, 0, 0))
    assert np.array_equal(got[0], render_ref.render_ball(ixyz, *c, r, h, w, (0, 0, 0)))


def test_all_points_on_one_pixel(ops):
    rng = np.random.RandomState(9)
    n = 5000
    ixyz = np.tile(np.array([[7, 9, 0]], np.int32), (n, 1))
    ixyz[:, 2] = rng.randint(-3, 4, n)
    c = rng.uniform(0, 255, (3, n)).astype(np.float32)
    for r in (1, 5):
        got = ball(ops, ixyz, c, r, 16, 20, (1, 2, 3))
        assert np.array_equal(got[0], render_ref.render_ball(ixyz, *c, r, 16, 20, (1, 2, 3))), r
        assert np.array_equal(got, ball(ops, ixyz, c, r, 16, 20, (1, 2, 3), dev="cpu")), r


def test_label_mode_with_out_of_range_labels(pn2, ops, palette):
    c = CALLS["direct_r4"]
    rng = np.random.RandomState(8)
    labels = rng.randint(0, 21, len(c["ixyz"])).astype(np.int32)
    labels[:4] = [-1, 21, 2 ** 31 - 1, -2 ** 31]
    looked = pn2.visualization.label_colors(t(labels), t(palette))
    assert looked.device.type == "cuda" and not looked[:4].any()
    bg = [int(b) for b in c["background"]]
    want = ball(ops, c["ixyz"], looked.cpu().numpy().T, 4, c["h"], c["w"], bg)
    got = ops.render_ball(t(c["ixyz"][None]), None, None, None, t(labels), t(palette), 4, c["h"],
                          c["w"], bg)
    assert np.array_equal(got.cpu().numpy(), want)
    host = ops.render_ball(t(c["ixyz"][None], "cpu"), None, None, None, t(labels, "cpu"),
                           t(palette, "cpu"), 4, c["h"], c["w"], bg)
    assert np.array_equal(host.numpy(), want)


def test_n0_gives_the_background(ops):
    got = ops.render_ball(torch.zeros(2, 0, 3, dtype=torch.int32, device=DEV),
                          *[torch.zeros(0, device=DEV)] * 3, None, None, 5, 6, 7, [10, 20, 30])
    assert got.shape == (2, 6, 7, 3)
    assert (got.cpu().numpy() == np.array([10, 20, 30], np.uint8)).all()


def test_meta_agrees_with_the_device(ops):
    c = CALLS["direct_r4"]
    n = len(c["ixyz"])
    ball_args = (t(np.stack([c["ixyz"]] * 2)), t(c["c"][0]), t(c["c"][1]), t(c["c"][2]), None, None,
                 4, c["h"], c["w"], [0, 0, 0])
    proj_args = (t(np.zeros((n, 3), np.float32)), t(np.zeros((3, 12))))
    for op, args in ((ops.render_ball, ball_args), (ops.render_project, proj_args)):
        real = op(*args)
        fake = op(*[a.to("meta") if isinstance(a, torch.Tensor) else a for a in args])
        assert fake.device.type == "meta"
        assert (fake.shape, fake.dtype, fake.stride()) == (real.shape, real.dtype, real.stride())


def test_animate_prediction_on_the_device(pn2, palette, tmp_path):
    v = pn2.visualization
    rng = np.random.RandomState(4)
    n = 3000
    result = {"points": t(rng.rand(n, 3).astype(np.float32)),
              "labels": t(rng.randint(1, 21, n).astype(np.int32)),
              "gt_labels": t(rng.randint(0, 21, n).astype(np.int32))}
    kw = dict(size=(48, 64), ballradius=3)
    written = v.animate_prediction(result, palette, str(tmp_path), name="scene0002_00",
                                   n_frames=4, **kw)
    for sub in ("groundtruth", "predictions"):
        want = [str(tmp_path / sub / "scene0002_00" / ("frame_%03d.png" % k)) for k in range(4)]
        assert written[sub] == want and all(os.path.exists(q) for q in want)
    from PIL import Image
    xa, ya = zip(*v.orbit(4))
    masked = v.mask_unannotated(result["labels"], result["gt_labels"])
    frames = v.render_scene(result["points"], masked, palette, xangle=xa, yangle=ya, **kw)
    assert frames.device.type == "cuda" and frames.shape == (4, 48, 64, 3)
    host = v.render_scene(result["points"].cpu(), masked.cpu(), palette, xangle=xa, yangle=ya,
                          device="cpu", **kw)
    assert np.array_equal(frames.cpu().numpy(), host.numpy())
    disk = np.asarray(Image.open(written["predictions"][2]).convert("RGB"))
    assert np.array_equal(disk, frames[2].cpu().numpy()[..., ::-1])
