"""visualization — looking at a labelled scene (attention_points/visualization/
qualitative_animations.py and labels_during_training.py), headless and on the device.

The reference colours a scene's points by ground-truth and by predicted label, blackens the
predictions where the ground truth is unannotated, and records rotating views with pptk. Here
the same pictures come from the ball renderer of show3d_balls (csrc/render.hip): labels go to
the kernel with a palette and are looked up once per pixel, and all frames of an orbit are
rendered in a few launches. The palette and the label names are arguments: the reference's
table is data of its own (tests/golden/render/palette.json holds it for the tests).

Not reproduced: pptk's perspective camera and its key-frame interpolation (view.record's poses).
pptk cannot be installed where this runs and the reference keeps no rendered image, so there is
nothing to compare with. The camera is show3d_balls' orthographic one: orbit() turns it once
around the vertical axis at a fixed elevation, which is what the reference's five poses
(phi = 0 .. 2 pi, theta = pi / 4) describe.

Frames are written as PNG with PIL when it imports and as binary PPM otherwise, under the file
names the reference's ffmpeg line expects (groundtruth/NAME/frame_%03d.png, predictions/NAME/
frame_%03d.png). The renderer's channel order is OpenCV's (blue, green, red); the writer reverses
it, so a file shows what cv2.imwrite would have stored.
"""
import os

import numpy as np
import torch

from . import show3d_balls

WHITE = (255, 255, 255)  # the reference's bg_color


def _as_tensor(a, dev, dtype):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def label_colors(labels, palette):
    """colors[i] = palette[labels[i]] (the reference's map over g_label_colors), (n, 3) float32 on
    labels' device; a label outside the palette takes row 0, as in the renderer."""
    dev = labels.device if isinstance(labels, torch.Tensor) else torch.device("cpu")
    pal = _as_tensor(palette, dev, torch.float32)
    lab = _as_tensor(labels, dev, torch.int64).reshape(-1)
    lab = torch.where((lab >= 0) & (lab < pal.shape[0]), lab, torch.zeros_like(lab))
    return pal[lab]


def mask_unannotated(pred, gt):
    """animate_scenes' blackening: a point keeps its prediction where gt != 0 and gets label 0
    (unannotated, black) elsewhere."""
    if isinstance(pred, torch.Tensor):
        gt = _as_tensor(gt, pred.device, torch.int64).reshape(pred.shape)
        return torch.where(gt != 0, pred, torch.zeros_like(pred))
    pred, gt = np.asarray(pred), np.asarray(gt)
    return np.where(gt != 0, pred, np.zeros_like(pred))


def orbit(n_frames, elevation=np.pi / 4):
    """The (xangle, yangle) pairs of one full turn in n_frames steps at a fixed elevation:
    (elevation, 2 pi k / n_frames)."""
    if n_frames < 1:
        raise ValueError(f"orbit expects n_frames >= 1, got {n_frames}")
    return [(float(elevation), 2.0 * np.pi * k / n_frames) for k in range(n_frames)]


def render_scene(points, labels, palette, xangle=0.0, yangle=0.0, zoom=1.0, size=(800, 800),
                 ballradius=10, background=WHITE, device=None):
    """A scene coloured by label: (h, w, 3) uint8 on the device for scalar angles and zoom,
    (F, h, w, 3) for sequences. points (n, 3), labels (n), palette (npal, 3) in 0..255."""
    h, w = int(size[0]), int(size[1])
    dev = show3d_balls._device_of(points if isinstance(points, torch.Tensor) else labels, device)
    xyz = torch.from_numpy(show3d_balls.prepare(points, min(h, w))).to(dev)
    lab = _as_tensor(labels, dev, torch.int32).reshape(-1)
    if lab.shape[0] != xyz.shape[0]:
        raise ValueError(f"render_scene expects one label per point, got {lab.shape[0]} labels "
                         f"for {xyz.shape[0]} points")
    single = all(np.ndim(v) == 0 for v in (xangle, yangle, zoom))
    mats = show3d_balls.view_matrices(xangle, yangle, zoom, h, w)
    show = show3d_balls.render(xyz, mats, h, w, ballradius, background, labels=lab,
                               palette=_as_tensor(palette, dev, torch.float32))
    return show[0] if single else show


def write_frame(path, image):
    """One (h, w, 3) uint8 frame in the renderer's (blue, green, red) order to `path`, channels
    reversed: PNG through PIL when it imports, else binary PPM under the same name with .ppm.
    Returns the path written."""
    rgb = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    rgb = np.ascontiguousarray(rgb[..., ::-1], np.uint8)
    try:
        from PIL import Image
    except ImportError:
        path = os.path.splitext(path)[0] + ".ppm"
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
            f.write(rgb.tobytes())
        return path
    Image.fromarray(rgb).save(path)
    return path


def write_frames(directory, frames):
    """frames (F, h, w, 3) as directory/frame_000.png, frame_001.png, ...; returns the paths."""
    os.makedirs(directory, exist_ok=True)
    host = frames.detach().cpu() if isinstance(frames, torch.Tensor) else frames
    return [write_frame(os.path.join(directory, "frame_%03d.png" % k), host[k])
            for k in range(len(host))]


def animate_prediction(result, palette, out_dir, name="scene", n_frames=120,
                       elevation=np.pi / 4, zoom=1.0, size=(800, 800), ballradius=10,
                       background=WHITE):
    """qualitative_animations.animate_scenes for one scene: `result` is predict_scene's dictionary
    ('points', 'labels' and, when the scene had labels, 'gt_labels', device tensors). Renders one
    orbit of the ground truth and one of the prediction, blackened where the ground truth is
    unannotated, and writes out_dir/groundtruth/NAME/frame_%03d.png and out_dir/predictions/NAME/
    frame_%03d.png. Without 'gt_labels' only the prediction is written, unmasked. Returns
    {'groundtruth': [paths], 'predictions': [paths]}."""
    xa, ya = zip(*orbit(n_frames, elevation))
    points, pred = result["points"], result["labels"]
    written = {"groundtruth": [], "predictions": []}
    kw = dict(xangle=xa, yangle=ya, zoom=zoom, size=size, ballradius=ballradius,
              background=background)
    if "gt_labels" in result:
        gt = result["gt_labels"]
        written["groundtruth"] = write_frames(os.path.join(out_dir, "groundtruth", name),
                                              render_scene(points, gt, palette, **kw))
        pred = mask_unannotated(pred, gt)
    written["predictions"] = write_frames(os.path.join(out_dir, "predictions", name),
                                          render_scene(points, pred, palette, **kw))
    return written


def labels_over_training(points, label_sets, palette, xangle=np.pi / 4, yangle=0.0, zoom=1.0,
                         size=(800, 800), ballradius=10, background=WHITE, device=None):
    """labels_during_training.animate_prediction_changes: one view of the scene per checkpoint's
    labels, (len(label_sets), h, w, 3) uint8 on the device. The scene is prepared and projected
    once per call of the renderer; only the labels change."""
    h, w = int(size[0]), int(size[1])
    dev = show3d_balls._device_of(points, device)
    xyz = torch.from_numpy(show3d_balls.prepare(points, min(h, w))).to(dev)
    mats = show3d_balls.view_matrices(float(xangle), float(yangle), float(zoom), h, w)
    pal = _as_tensor(palette, dev, torch.float32)
    views = [show3d_balls.render(xyz, mats, h, w, ballradius, background,
                                 labels=_as_tensor(l, dev, torch.int32).reshape(-1), palette=pal)
             for l in label_sets]
    if not views:
        return torch.empty((0, h, w, 3), dtype=torch.uint8, device=dev)
    return torch.cat(views)
