"""show3d_balls — the reference's point-cloud viewer (pointnet2_tensorflow/utils/
show3d_balls.py), headless: showpoints returns the image(s) it would have put in its window.

The viewer draws every point as a shaded ball with its native render_ball and turns the scene with
the mouse. An MI355X box has no display, so the window, the mouse and the key loop are replaced
by explicit arguments: `xangle`, `yangle` and `zoom` (what the mouse position and the n / m keys
set; scalars, or sequences for several frames), `showsz` or `size=(h, w)`, and `which` = "gt" or
"pred" (the t / p keys). The projection and the renderer are the kernels of csrc/render.hip
(torch.ops.pn2.render_project, render_ball; CPU tensors run the host twins): the images equal the
reference's bit for bit (tests/golden/make_golden_render.py).

Per scene, once, on the host in numpy, as the reference writes it: centre by the mean, scale by
2.2 * max norm / showsz. The result is uploaded once; everything per frame (projection, splat,
shading, magnifyBlue) runs on the device, F frames per launch.
"""
import numpy as np
import torch

from . import _torch_ops

showsz = 800  # the reference's module-level default
MAX_CHUNK_BYTES = 256 << 20  # key buffers (8 h w per frame) and projected points (12 n per frame)


def prepare(xyz, showsz):
    """The viewer's preamble (show3d_balls.py:27-29) in numpy, in xyz's own dtype: the points
    centred by their mean and scaled so that the farthest lies at showsz / 2.2 pixels."""
    if isinstance(xyz, torch.Tensor):
        xyz = xyz.detach().cpu().numpy()
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64):
        xyz = xyz.astype(np.float64)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"showpoints expects (n, 3) xyz, got {xyz.shape}")
    if len(xyz) == 0:
        return xyz.copy()
    xyz = xyz - xyz.mean(axis=0)
    radius = ((xyz ** 2).sum(axis=-1) ** 0.5).max()
    xyz /= (radius * 2.2) / showsz
    return xyz


def view_matrices(xangle, yangle, zoom, h, w):
    """(F, 12) float64: per frame the viewer's rotmat (a turn about x by xangle, then about y by
    yangle, times zoom; :52-71) row-major, then the offset (h / 2, w / 2, 0). Scalars broadcast
    against sequences. Every entry of the product has one non-zero term, so it is the same bits
    however the 3 x 3 product is summed."""
    xa, ya, zm = np.broadcast_arrays(np.atleast_1d(np.asarray(xangle, np.float64)),
                                     np.atleast_1d(np.asarray(yangle, np.float64)),
                                     np.atleast_1d(np.asarray(zoom, np.float64)))
    mats = np.empty((len(xa), 12), np.float64)
    for f, (a, b, z) in enumerate(zip(xa, ya, zm)):
        rx = np.array([[1.0, 0.0, 0.0],
                       [0.0, np.cos(a), -np.sin(a)],
                       [0.0, np.sin(a), np.cos(a)]])
        ry = np.array([[np.cos(b), 0.0, -np.sin(b)],
                       [0.0, 1.0, 0.0],
                       [np.sin(b), 0.0, np.cos(b)]])
        rot = np.eye(3).dot(rx).dot(ry)
        rot *= z
        mats[f, :9] = rot.reshape(9)
        mats[f, 9:] = (h / 2, w / 2, 0.0)
    return mats


def render(xyz, mats, h, w, ballradius=10, background=(0, 0, 0), channels=None, labels=None,
           palette=None):
    """F frames of one prepared scene. xyz (n, 3) float32 / float64 on the rendering device; mats
    (F, 12) numpy (view_matrices); channels = (c0, c1, c2), three (n) float32 tensors, or labels
    (n) int32 and palette (npal, 3) float32. Returns (F, h, w, 3) uint8 on xyz's device, in the
    reference's channel order (c2, c0, c1). F is cut into chunks whose key buffers and projected
    points stay under MAX_CHUNK_BYTES."""
    n, F = int(xyz.shape[0]), len(mats)
    per_frame = 8 * h * w + 12 * n + 1
    step = int(max(1, min(65535, MAX_CHUNK_BYTES // per_frame)))
    c0, c1, c2 = channels if channels is not None else (None, None, None)
    bg = [int(b) for b in background]
    out = []
    for f0 in range(0, F, step):
        m = torch.from_numpy(np.ascontiguousarray(mats[f0:f0 + step])).to(xyz.device)
        ixyz = _torch_ops.call("render_project", xyz, m)
        out.append(_torch_ops.call("render_ball", ixyz, c0, c1, c2, labels, palette,
                                   int(ballradius), int(h), int(w), bg))
    if not out:
        return torch.empty((0, h, w, 3), dtype=torch.uint8, device=xyz.device)
    return out[0] if len(out) == 1 else torch.cat(out)


def _device_of(xyz, device):
    if device is not None:
        return torch.device(device)
    if isinstance(xyz, torch.Tensor):
        return xyz.device
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _channels(colours, n, normalizecolor, dev):
    """The viewer's c0, c1, c2 (:30-48) as three contiguous float32 tensors on dev."""
    if colours is None:
        return tuple(torch.full((n,), 255.0, dtype=torch.float32, device=dev) for _ in range(3))
    c = colours if isinstance(colours, torch.Tensor) else torch.from_numpy(np.asarray(colours))
    if c.dim() != 2 or c.shape[0] != n or c.shape[1] != 3:
        raise ValueError(f"showpoints expects (n, 3) colours for {n} points, got {tuple(c.shape)}")
    c = c.to(device=dev, dtype=torch.float32)  # a copy or the caller's tensor: never written
    out = []
    for k in range(3):
        ch = c[:, k]
        if normalizecolor and n > 0:
            # c /= (c.max() + 1e-14) / 255.0, every step in float32
            d = np.float32(np.float32(ch.max().item()) + np.float32(1e-14)) / np.float32(255.0)
            ch = ch / float(d)
        out.append(ch.contiguous())
    return tuple(out)


def magnify_blue(show, magnifyBlue):
    """The reference's roll-and-maximum on channel 0 (:88-94), per frame, on the device."""
    if magnifyBlue <= 0:
        return show
    b = show[..., 0]
    b = torch.maximum(b, torch.roll(b, 1, dims=-2))
    if magnifyBlue >= 2:
        b = torch.maximum(b, torch.roll(b, -1, dims=-2))
    b = torch.maximum(b, torch.roll(b, 1, dims=-1))
    if magnifyBlue >= 2:
        b = torch.maximum(b, torch.roll(b, -1, dims=-1))
    show = show.clone()
    show[..., 0] = b
    return show


def showpoints(xyz, c_gt=None, c_pred=None, waittime=0, showrot=False, magnifyBlue=0,
               freezerot=False, background=(0, 0, 0), normalizecolor=True, ballradius=10, *,
               xangle=0.0, yangle=0.0, zoom=1.0, showsz=None, size=None, which="gt",
               device=None):
    """The image(s) the reference's showpoints would show: (h, w, 3) uint8 on the device for
    scalar xangle, yangle and zoom, (F, h, w, 3) when any of them is a sequence. Channels are in
    the reference's order, what cv2.imshow takes as blue, green, red: (c2, c0, c1) of the colour
    columns.

    xyz (n, 3) float32 or float64, numpy or tensor; c_gt / c_pred (n, 3) colours or None (white),
    chosen by which = "gt" | "pred". xangle = (mousey - 0.5) * pi * 1.2 and yangle = (mousex -
    0.5) * pi * 1.2 of the reference's mouse position; freezerot sets both to 0. The image is
    showsz x showsz (default: this module's showsz, 800), or size = (h, w), scaled by min(h, w).
    normalizecolor divides each channel by (max + 1e-14) / 255 in float32 (colours of another
    dtype are converted first). Colours are never modified: the reference normalises the
    caller's arrays in place, through views, and again on every t / p key; here they are only
    read. waittime is accepted and ignored (nothing waits); showrot, the text overlay, is not
    reproduced and raises. device: where to render (default: xyz's device if it is a tensor,
    else the GPU when there is one); CPU tensors run the host twins."""
    if showrot:
        raise NotImplementedError("showpoints: the showrot text overlay is not reproduced")
    if which not in ("gt", "pred"):
        raise ValueError(f"showpoints: which must be 'gt' or 'pred', got {which!r}")
    if size is None:
        side = int(globals()["showsz"] if showsz is None else showsz)
        h = w = side
    else:
        h, w = int(size[0]), int(size[1])
        side = min(h, w) if showsz is None else int(showsz)
    dev = _device_of(xyz, device)
    scaled = prepare(xyz, side)
    n = len(scaled)
    single = all(np.ndim(v) == 0 for v in (xangle, yangle, zoom))
    if freezerot:
        xangle, yangle = np.zeros_like(np.asarray(xangle, np.float64)), \
            np.zeros_like(np.asarray(yangle, np.float64))
    mats = view_matrices(xangle, yangle, zoom, h, w)
    channels = _channels(c_gt if which == "gt" else c_pred, n, normalizecolor, dev)
    show = render(torch.from_numpy(scaled).to(dev), mats, h, w, ballradius, background, channels)
    show = magnify_blue(show, magnifyBlue)
    return show[0] if single else show
