"""CPU: scene rendering (csrc/render.hip's host twins in csrc/cpu_render.cpp, the CPU kernels of
torch.ops.pn2.render_ball / render_project, show3d_balls.py, visualization.py).

The goldens are the reference's own output: its native render_ball driven by its viewer
(tests/golden/make_golden_render.py). Every comparison is exact, no pixel and no point left out.
tests/test_gpu_render.py compares the kernels with these twins on the MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import render_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "render")
E = -22
CALLS = render_ref.golden_calls(GOLDEN)


@pytest.fixture(scope="module")
def ops():
    import pn2hip
    return pn2hip.ops


@pytest.fixture(scope="module")
def palette():
    with open(os.path.join(GOLDEN, "palette.json")) as f:
        data = json.load(f)
    return np.array(data["label_colors"], np.float32), data["label_names"]


def p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def twin_ball(lib, ixyz, c, r, h, w, background, labels=None, pal=None):
    """pn2cpu_render_ball on numpy arrays: ixyz (F,n,3) or (n,3); returns (rc, images)."""
    ixyz = np.ascontiguousarray(ixyz, np.int32)
    ixyz = ixyz[None] if ixyz.ndim == 2 else ixyz
    F, n = ixyz.shape[:2]
    img = np.full((F, h, w, 3), 77, np.uint8)
    c = [None] * 3 if c is None else [np.ascontiguousarray(x, np.float32) for x in c]
    rc = lib.pn2cpu_render_ball(p(ixyz), F, n, p(c[0]), p(c[1]), p(c[2]), p(labels), p(pal),
                                0 if pal is None else len(pal), r, h, w,
                                *[int(b) for b in background], p(img))
    return rc, img


# ------------------------------------------------------------------ the reference's images
@pytest.mark.parametrize("name", sorted(CALLS))
def test_twin_reproduces_the_reference(pn2, name):
    c = CALLS[name]
    rc, img = twin_ball(pn2.lib(), c["ixyz"], c["c"], c["r"], c["h"], c["w"], c["background"])
    assert rc == 0
    assert np.array_equal(img[0], c["image"]), f"{(img[0] != c['image']).sum()} bytes differ"
    # and so does the numpy restatement the GPU tests use
    ref = render_ref.render_ball(c["ixyz"], *c["c"], c["r"], c["h"], c["w"], c["background"])
    assert np.array_equal(ref, c["image"])


@pytest.mark.parametrize("name", ["viewer_f32", "viewer_f64"])
def test_twin_projection_reproduces_the_reference(pn2, name):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    s = pn2.show3d_balls
    xyz = s.prepare(g["points"], int(g["showsz"]))
    assert xyz.dtype == g["points"].dtype
    mats = s.view_matrices(float(g["xangle"]), float(g["yangle"]), float(g["zoom"]), 96, 96)
    out = np.full((1, len(xyz), 3), -9, np.int32)
    assert pn2.lib().pn2cpu_render_project(p(xyz), int(xyz.dtype == np.float64), len(xyz),
                                           p(mats), 1, p(out)) == 0
    assert np.array_equal(out[0], g["ixyz"])
    assert np.array_equal(render_ref.project(xyz, mats[0]), g["ixyz"])


@pytest.mark.parametrize("name", ["viewer_f32", "viewer_f64"])
def test_showpoints_reproduces_the_viewer(pn2, name):
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    s = pn2.show3d_balls
    points, colours = torch.from_numpy(g["points"]), torch.from_numpy(g["colours"])
    kept = colours.clone()
    kw = dict(background=tuple(int(b) for b in g["background"]),
              normalizecolor=bool(g["normalizecolor"]), ballradius=int(g["ballradius"]),
              xangle=float(g["xangle"]), yangle=float(g["yangle"]), zoom=float(g["zoom"]),
              showsz=int(g["showsz"]))
    img = s.showpoints(points, colours, None, **kw)
    assert img.device.type == "cpu" and img.dtype == torch.uint8 and img.shape == (96, 96, 3)
    assert np.array_equal(img.numpy(), g["image"])
    assert torch.equal(colours, kept), "showpoints must not modify the caller's colours"
    # the normalised channels are the reference's, bit for bit
    ch = s._channels(colours, len(points), bool(g["normalizecolor"]), torch.device("cpu"))
    for k, c in enumerate(ch):
        assert np.array_equal(c.numpy().view(np.uint32), g[f"c{k}"].view(np.uint32)), f"c{k}"
    # numpy inputs, the colours as c_pred, the module-level default size
    s_showsz, s.showsz = s.showsz, int(g["showsz"])
    try:
        kw.pop("showsz")
        img2 = s.showpoints(g["points"], None, g["colours"], which="pred", device="cpu", **kw)
    finally:
        s.showsz = s_showsz
    assert np.array_equal(img2.numpy(), g["image"])


def test_showpoints_frames_white_and_magnify(pn2):
    g = np.load(os.path.join(GOLDEN, "viewer_f32.npz"))
    s = pn2.show3d_balls
    pts = torch.from_numpy(g["points"])
    kw = dict(ballradius=2, size=(40, 56), background=(9, 9, 9))
    xa, ya = [0.2, -0.4, 1.0], [0.0, 0.5, 2.0]
    frames = s.showpoints(pts, xangle=xa, yangle=ya, zoom=1.3, **kw)
    assert frames.shape == (3, 40, 56, 3)
    for f in range(3):
        one = s.showpoints(pts, xangle=xa[f], yangle=ya[f], zoom=1.3, **kw)
        assert torch.equal(frames[f], one)
    # c_gt None is white: three equal channels
    assert torch.equal(frames[..., 0], frames[..., 1]) and torch.equal(frames[..., 0], frames[..., 2])
    frozen = s.showpoints(pts, xangle=0.7, yangle=0.3, freezerot=True, **kw)
    assert torch.equal(frozen, s.showpoints(pts, **kw))
    # chunking F changes nothing
    chunk, s.MAX_CHUNK_BYTES = s.MAX_CHUNK_BYTES, 1
    try:
        assert torch.equal(s.showpoints(pts, xangle=xa, yangle=ya, zoom=1.3, **kw), frames)
    finally:
        s.MAX_CHUNK_BYTES = chunk
    # magnifyBlue is the reference's roll-and-maximum on channel 0
    base = frames[0].numpy()
    for level in (1, 2):
        show = base.copy()
        show[:, :, 0] = np.maximum(show[:, :, 0], np.roll(show[:, :, 0], 1, axis=0))
        if level >= 2:
            show[:, :, 0] = np.maximum(show[:, :, 0], np.roll(show[:, :, 0], -1, axis=0))
        show[:, :, 0] = np.maximum(show[:, :, 0], np.roll(show[:, :, 0], 1, axis=1))
        if level >= 2:
            show[:, :, 0] = np.maximum(show[:, :, 0], np.roll(show[:, :, 0], -1, axis=1))
        got = s.showpoints(pts, xangle=xa[0], yangle=ya[0], zoom=1.3, magnifyBlue=level, **kw)
        assert np.array_equal(got.numpy(), show)
    with pytest.raises(NotImplementedError):
        s.showpoints(pts, showrot=True, **kw)
    with pytest.raises(ValueError):
        s.showpoints(pts, which="both", **kw)
    with pytest.raises(ValueError):
        s.showpoints(pts, torch.zeros(5, 3), **kw)


# ------------------------------------------------------------------ the op on CPU tensors
def test_op_equals_twin_and_frames_are_independent(pn2, ops):
    c = CALLS["direct_r4"]
    rng = np.random.RandomState(3)
    shift = rng.randint(-6, 7, (3, 1, 3)).astype(np.int32)
    ixyz = c["ixyz"][None] + shift  # three frames
    rc, want = twin_ball(pn2.lib(), ixyz, c["c"], 4, c["h"], c["w"], c["background"])
    assert rc == 0
    t = torch.from_numpy
    ch = [t(x) for x in c["c"]]
    bg = [int(b) for b in c["background"]]
    got = ops.render_ball(t(ixyz), *ch, None, None, 4, c["h"], c["w"], bg)
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want)
    for f in range(3):
        one = ops.render_ball(t(ixyz[f:f + 1].copy()), *ch, None, None, 4, c["h"], c["w"], bg)
        assert np.array_equal(one.numpy()[0], want[f])
        assert np.array_equal(want[f], render_ref.render_ball(ixyz[f], *c["c"], 4, c["h"], c["w"],
                                                              c["background"]))
    # strided and offset inputs give the contiguous result
    wide = torch.zeros(3, len(c["ixyz"]), 5, dtype=torch.int32)
    wide[:, :, 1:4] = t(ixyz)
    cols = t(np.ascontiguousarray(c["c"].T))  # (n, 3): each channel has stride 3
    got2 = ops.render_ball(wide[:, :, 1:4], cols[:, 0], cols[:, 1], cols[:, 2], None, None, 4,
                           c["h"], c["w"], bg)
    assert np.array_equal(got2.numpy(), want)


def test_label_mode_equals_colour_mode(pn2, ops, palette):
    pal, names = palette
    assert len(names) == len(pal) == 21 and names[0] == "unannotated" and not pal[0].any()
    c = CALLS["direct_r4"]
    rng = np.random.RandomState(8)
    labels = rng.randint(0, 21, len(c["ixyz"])).astype(np.int32)
    labels[:4] = [-1, 21, 2 ** 31 - 1, -2 ** 31]  # out of range: row 0
    looked = pn2.visualization.label_colors(labels, pal).numpy()
    assert np.array_equal(looked[4:], pal[labels[4:]]) and not looked[:4].any()
    rc, want = twin_ball(pn2.lib(), c["ixyz"], looked.T, 4, c["h"], c["w"], c["background"])
    rc2, got = twin_ball(pn2.lib(), c["ixyz"], None, 4, c["h"], c["w"], c["background"],
                         labels=labels, pal=pal)
    assert rc == 0 and rc2 == 0 and np.array_equal(got, want)
    t = torch.from_numpy
    op = ops.render_ball(t(c["ixyz"][None].copy()), None, None, None, t(labels), t(pal), 4, c["h"],
                         c["w"], [int(b) for b in c["background"]])
    assert np.array_equal(op.numpy(), want)


def test_colours_are_clamped(pn2):
    ixyz = np.array([[3, 3, 0], [3, 9, 0], [9, 3, 0], [9, 9, 0]], np.int32)
    wild = np.array([[-5.0, 300.0, np.nan, 255.5]] * 3, np.float32)
    tame = np.array([[0.0, 255.0, 0.0, 255.0]] * 3, np.float32)
    a = twin_ball(pn2.lib(), ixyz, wild, 3, 13, 13, (1, 1, 1))
    b = twin_ball(pn2.lib(), ixyz, tame, 3, 13, 13, (1, 1, 1))
    assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1])


def test_n0_and_empty(pn2, ops):
    rc, img = twin_ball(pn2.lib(), np.zeros((2, 0, 3), np.int32), None, 5, 6, 7, (10, 20, 30))
    assert rc == 0 and (img == np.array([10, 20, 30], np.uint8)).all()
    got = ops.render_ball(torch.zeros(2, 0, 3, dtype=torch.int32), *[torch.zeros(0)] * 3, None, None,
                          5, 6, 7, [10, 20, 30])
    assert got.shape == (2, 6, 7, 3) and np.array_equal(got.numpy(), img)
    assert ops.render_ball(torch.zeros(0, 4, 3, dtype=torch.int32), *[torch.zeros(4)] * 3, None,
                           None, 5, 6, 7, [0, 0, 0]).shape == (0, 6, 7, 3)
    assert ops.render_project(torch.zeros(0, 3), torch.zeros(2, 12, dtype=torch.float64)).shape == \
        (2, 0, 3)
    assert ops.render_project(torch.zeros(5, 3), torch.zeros(0, 12, dtype=torch.float64)).shape == \
        (0, 5, 3)
    assert pn2.show3d_balls.showpoints(np.zeros((0, 3), np.float32), size=(4, 5), device="cpu",
                                       background=(1, 2, 3)).shape == (4, 5, 3)


def test_projection_op_and_saturation(pn2, ops):
    rng = np.random.RandomState(2)
    mats = pn2.show3d_balls.view_matrices([0.3, -1.0], [0.9, 2.5], [1.0, 0.7], 64, 48)
    for dtype in (np.float32, np.float64):
        xyz = (rng.randn(300, 3) * 40).astype(dtype)
        got = ops.render_project(torch.from_numpy(xyz), torch.from_numpy(mats)).numpy()
        assert got.dtype == np.int32 and got.shape == (2, 300, 3)
        for f in range(2):
            assert np.array_equal(got[f], render_ref.project(xyz, mats[f]))
        # a strided xyz and a mats view give the same
        wide = torch.zeros(300, 7, dtype=torch.from_numpy(xyz).dtype)
        wide[:, 2:5] = torch.from_numpy(xyz)
        mwide = torch.zeros(2, 14, dtype=torch.float64)
        mwide[:, 1:13] = torch.from_numpy(mats)
        assert np.array_equal(ops.render_project(wide[:, 2:5], mwide[:, 1:13]).numpy(), got)
    big = np.array([[3e9, -3e9, np.nan], [2147483647.5, -2147483648.5, 0.75]], np.float64)
    ident = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float64)
    got = ops.render_project(torch.from_numpy(big), torch.from_numpy(ident)).numpy()[0]
    lo = -2 ** 31
    assert got.tolist() == [[lo, lo, lo], [2147483647, lo, 0]]


def test_argument_errors(pn2, ops):
    lib = pn2.lib()
    ixyz, c = np.zeros((1, 2, 3), np.int32), np.zeros((3, 2), np.float32)
    ok = twin_ball(lib, ixyz, c, 2, 4, 4, (0, 0, 0))
    assert ok[0] == 0
    assert twin_ball(lib, ixyz, c, 32768, 4, 4, (0, 0, 0))[0] == E
    assert twin_ball(lib, ixyz, c, 2, 4, 4, (0, 256, 0))[0] == E
    assert twin_ball(lib, ixyz, c, 2, 4, 4, (0, -1, 0))[0] == E
    assert twin_ball(lib, ixyz, None, 2, 4, 4, (0, 0, 0))[0] == E
    assert twin_ball(lib, ixyz, None, 2, 4, 4, (0, 0, 0), labels=np.zeros(2, np.int32))[0] == E
    assert twin_ball(lib, ixyz, c, 2, 65536, 65536, (0, 0, 0))[0] == E
    img = np.zeros(48, np.uint8)
    assert lib.pn2cpu_render_ball(p(ixyz), -1, 2, p(c[0]), p(c[1]), p(c[2]), None, None, 0, 2, 4, 4,
                                  0, 0, 0, p(img)) == E
    assert lib.pn2cpu_render_ball(p(ixyz), 1, 1 << 31, p(c[0]), p(c[1]), p(c[2]), None, None, 0, 2,
                                  4, 4, 0, 0, 0, p(img)) == E
    assert lib.pn2cpu_render_ball(p(ixyz), 1, 2, p(c[0]), p(c[1]), p(c[2]), None, None, 0, 2, 4, 4,
                                  0, 0, 0, None) == E
    assert lib.pn2cpu_render_project(None, 0, 2, p(np.zeros(12)), 1, p(ixyz)) == E
    assert lib.pn2cpu_render_project(p(c), 0, -1, p(np.zeros(12)), 1, p(ixyz)) == E
    # the device entry points check before any launch (no GPU needed: nothing is launched)
    assert lib.pn2_render_ball(16, 1, 2, 16, 16, 16, None, None, 0, 32768, 4, 4, 0, 0, 0, 16, 16,
                               1 << 20, None) == E
    assert lib.pn2_render_ball(16, 1, 2, 16, 16, 16, None, None, 0, 2, 4, 4, 0, 0, 0, 16, 16,
                               8, None) == E  # workspace too small
    assert lib.pn2_render_ball(16, 1, 2, 16, 16, 16, None, None, 0, 2, 4, 4, 0, 0, 0, 16, 12,
                               1 << 20, None) == E  # workspace misaligned
    assert lib.pn2_render_ball(16, 1, 2, 16, 16, 16, 16, None, 0, 2, 4, 4, 0, 0, 0, 16, 16,
                               1 << 20, None) == E  # labels without a palette
    assert lib.pn2_render_ball(None, 0, 2, None, None, None, None, None, 0, 2, 4, 4, 0, 0, 0, None,
                               None, 0, None) == 0  # F = 0
    assert lib.pn2_render_ball_workspace_size(3, 4, 5) == (3 * 4 * 5 + 6) * 8
    assert lib.pn2_render_project(16, 0, 2, 12, 1, 16, None) == E  # mats misaligned
    assert lib.pn2_render_project(16, 0, 1 << 31, 16, 1, 16, None) == E
    assert lib.pn2_render_project(None, 0, 0, None, 1, None, None) == 0
    # the ops' own checks
    z = torch.zeros
    i3 = z(1, 2, 3, dtype=torch.int32)
    ch = [z(2)] * 3
    bad = [
        lambda: ops.render_ball(z(2, 3, dtype=torch.int32), *ch, None, None, 2, 4, 4, [0, 0, 0]),
        lambda: ops.render_ball(z(1, 2, 3), *ch, None, None, 2, 4, 4, [0, 0, 0]),
        lambda: ops.render_ball(i3, z(3), z(2), z(2), None, None, 2, 4, 4, [0, 0, 0]),
        lambda: ops.render_ball(i3, *ch, None, None, 2, 4, 4, [0, 0]),
        lambda: ops.render_ball(i3, *ch, None, None, 2, 4, 4, [0, 0, 256]),
        lambda: ops.render_ball(i3, *ch, None, None, 2, -1, 4, [0, 0, 0]),
        lambda: ops.render_ball(i3, *ch, None, None, 32768, 4, 4, [0, 0, 0]),
        lambda: ops.render_ball(i3, *ch, z(2, dtype=torch.int32), z(5, 3), 2, 4, 4, [0, 0, 0]),
        lambda: ops.render_ball(i3, None, None, None, z(2, dtype=torch.int32), None, 2, 4, 4,
                                [0, 0, 0]),
        lambda: ops.render_ball(i3, None, None, None, z(2, dtype=torch.int32), z(0, 3), 2, 4, 4,
                                [0, 0, 0]),
        lambda: ops.render_project(z(4, 2), z(1, 12, dtype=torch.float64)),
        lambda: ops.render_project(z(4, 3), z(1, 12)),
        lambda: ops.render_project(z(4, 3, dtype=torch.int32), z(1, 12, dtype=torch.float64)),
        lambda: ops.render_project(z(4, 3), z(1, 9, dtype=torch.float64)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {k} passed")


def test_schemas_kernels_and_exports(pn2, ops):
    import pn2hip
    assert ops.RENDER_NAMES == ("render_ball", "render_project")
    for name in ops.RENDER_NAMES:
        assert name in ops.__all__ and name not in ops.NAMES + ops.HOST_NAMES
        for key in ("CPU", "CUDA", "Meta"):
            assert torch._C._dispatch_has_kernel_for_dispatch_key(f"pn2::{name}", key), (name, key)
    assert str(ops.render_ball._schemas[""]) == (
        "pn2::render_ball(Tensor ixyz, Tensor? c0, Tensor? c1, Tensor? c2, Tensor? labels, "
        "Tensor? palette, int r, int h, int w, int[] background) -> Tensor")
    assert str(ops.render_project._schemas[""]) == \
        "pn2::render_project(Tensor xyz, Tensor mats) -> Tensor"
    for name in ("show3d_balls", "visualization"):
        assert name in pn2.__all__ and name in pn2hip.__all__ and hasattr(pn2hip, name)
    m = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device="meta")  # noqa: E731
    out = ops.render_ball(m(3, 9, 3, dt=torch.int32), m(9), m(9), m(9), None, None, 2, 5, 6, [0, 0, 0])
    assert out.shape == (3, 5, 6, 3) and out.dtype == torch.uint8 and out.device.type == "meta"
    out = ops.render_project(m(9, 3, dt=torch.float64), m(4, 12, dt=torch.float64))
    assert out.shape == (4, 9, 3) and out.dtype == torch.int32


# ------------------------------------------------------------------ visualization
def test_mask_unannotated_and_orbit(pn2):
    v = pn2.visualization
    pred, gt = np.array([3, 4, 5, 0, 7]), np.array([1, 0, 2, 0, 0])
    assert v.mask_unannotated(pred, gt).tolist() == [3, 0, 5, 0, 0]
    got = v.mask_unannotated(torch.tensor(pred, dtype=torch.int32), torch.tensor(gt))
    assert got.dtype == torch.int32 and got.tolist() == [3, 0, 5, 0, 0]
    turn = v.orbit(8, 0.5)
    assert len(turn) == 8 and turn[0] == (0.5, 0.0) and all(a == 0.5 for a, _ in turn)
    assert np.allclose([b for _, b in turn], np.arange(8) * np.pi / 4)
    assert v.orbit(3)[0][0] == np.pi / 4
    with pytest.raises(ValueError):
        v.orbit(0)


def test_frame_writer_names_and_channel_order(pn2, tmp_path):
    v = pn2.visualization
    frames = np.zeros((2, 3, 4, 3), np.uint8)
    frames[0, 1, 2] = (10, 20, 30)  # blue, green, red, as cv2 holds an image
    frames[1, 0, 0] = (200, 100, 50)
    paths = v.write_frames(str(tmp_path / "groundtruth" / "scene0000_00"), torch.from_numpy(frames))
    assert [os.path.basename(q) for q in paths] == ["frame_000.png", "frame_001.png"]
    from PIL import Image
    rgb = np.asarray(Image.open(paths[0]).convert("RGB"))
    assert rgb.shape == (3, 4, 3) and rgb[1, 2].tolist() == [30, 20, 10] and rgb.sum() == 60
    assert np.asarray(Image.open(paths[1]))[0, 0].tolist() == [50, 100, 200]


def test_animate_prediction_and_training_views(pn2, palette, tmp_path):
    v = pn2.visualization
    pal, _ = palette
    rng = np.random.RandomState(4)
    n = 400
    points = torch.from_numpy(rng.rand(n, 3).astype(np.float32))
    gt = torch.from_numpy(rng.randint(0, 21, n).astype(np.int32))
    pred = torch.from_numpy(rng.randint(1, 21, n).astype(np.int32))
    result = {"points": points, "labels": pred, "gt_labels": gt}
    kw = dict(size=(24, 32), ballradius=2)
    written = v.animate_prediction(result, pal, str(tmp_path), name="scene0001_00", n_frames=3, **kw)
    for sub in ("groundtruth", "predictions"):
        want = [str(tmp_path / sub / "scene0001_00" / ("frame_%03d.png" % k)) for k in range(3)]
        assert written[sub] == want and all(os.path.exists(q) for q in want)
    # frame 1 of the prediction is the masked labels seen from the orbit's second view
    from PIL import Image
    xa, ya = v.orbit(3)[1]
    masked = v.mask_unannotated(pred, gt)
    view = v.render_scene(points, masked, pal, xangle=xa, yangle=ya, **kw).numpy()
    assert view.shape == (24, 32, 3)
    disk = np.asarray(Image.open(written["predictions"][1]).convert("RGB"))
    assert np.array_equal(disk, view[..., ::-1])
    # label mode is colour mode on the looked-up colours, through the viewer's entry point too
    colours = v.label_colors(masked, pal)
    same = pn2.show3d_balls.showpoints(points, colours, normalizecolor=False, xangle=xa, yangle=ya,
                                       background=v.WHITE, **kw)
    assert np.array_equal(same.numpy(), view)
    only = v.animate_prediction({"points": points, "labels": pred}, pal, str(tmp_path / "b"),
                                n_frames=2, **kw)
    assert only["groundtruth"] == [] and len(only["predictions"]) == 2
    views = v.labels_over_training(points, [gt, pred, masked], pal, **kw)
    assert views.shape == (3, 24, 32, 3)
    assert np.array_equal(views[2].numpy(),
                          v.render_scene(points, masked, pal, xangle=np.pi / 4, **kw).numpy())
