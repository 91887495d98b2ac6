#!/usr/bin/env python3
"""Golden vectors of the ball renderer, made by the REFERENCE's own code: its native
render_ball (pointnet2_tensorflow/utils/render_balls_so.cpp, compiled here with g++ into a
temporary directory) driven by its viewer (utils/show3d_balls.py showpoints) with a stub `cv2`
and np.ctypeslib.load_library redirected to that library. Only the .npz / .json written to
tests/golden/render/ are kept; the library goes with the temporary directory. (A directory of
their own: tests/test_oracle_golden.py takes every tests/golden/*.npz for an oracle case.)

  viewer_f32.npz   (a) 700 float32 points, 96 x 96, radius 3, a non-black background,
                   random colours, normalizecolor=True: the viewer's inputs (points,
                   colours, mousex / mousey and the angles they mean, zoom) and what
                   reaches render_ball and comes back (h, w, r, ixyz, c0, c1, c2,
                   background, image)
  viewer_f64.npz   (b) the same with float64 points and normalizecolor=False
  direct.npz       (c) render_ball called directly on a 48 x 80 image with one point set
                   at r = 0 (clamps to 1), r = 4 and r = 40: identical points with
                   different colours, different points that reach one pixel at equal z2,
                   points clipped by each border and each corner, points wholly outside,
                   negative z
  n1.npz           (d) n = 1
  palette.json     (e) the label names and colours of attention_points/visualization/
                   qualitative_animations.py, read as data (the module itself needs pptk)

Run: python tests/golden/make_golden_render.py <root of the reference checkout>
"""
import ast
import ctypes
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "render")
VIEWER_SEED = 11  # change the seed, not the rule, if a regenerated case stops being exact


class Recorder:
    """Stands where the viewer expects its ctypes library; keeps each render_ball call."""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def render_ball(self, h, w, show, n, ixyz, c0, c1, c2, r):
        h_, w_, n_, r_ = h.value, w.value, n.value, r.value
        arr = lambda p, ct, count: np.ctypeslib.as_array(  # noqa: E731
            ctypes.cast(p, ctypes.POINTER(ct)), (count,)).copy()
        call = {"h": h_, "w": w_, "r": r_,
                "ixyz": arr(ixyz, ctypes.c_int32, n_ * 3).reshape(n_, 3),
                "c0": arr(c0, ctypes.c_float, n_), "c1": arr(c1, ctypes.c_float, n_),
                "c2": arr(c2, ctypes.c_float, n_),
                "background": arr(show, ctypes.c_uint8, 3)}
        self.lib.render_ball(h, w, show, n, ixyz, c0, c1, c2, r)
        call["image"] = arr(show, ctypes.c_uint8, h_ * w_ * 3).reshape(h_, w_, 3)
        self.calls.append(call)


def load_viewer(root, lib):
    """The reference's show3d_balls module over a stub cv2 and the recorder."""
    cv2 = types.ModuleType("cv2")
    for name in ("namedWindow", "moveWindow", "setMouseCallback", "imshow", "imwrite", "putText"):
        setattr(cv2, name, lambda *a, **k: None)
    cv2.waitKey = lambda *a: -1
    sys.modules["cv2"] = cv2
    rec = Recorder(lib)
    real = np.ctypeslib.load_library
    np.ctypeslib.load_library = lambda *a, **k: rec
    try:
        spec = importlib.util.spec_from_file_location(
            "reference_show3d_balls",
            os.path.join(root, "pointnet2_tensorflow", "utils", "show3d_balls.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        np.ctypeslib.load_library = real
        del sys.modules["cv2"]
    return mod, rec


def viewer_case(mod, rec, dtype, normalizecolor, path):
    rng = np.random.RandomState(VIEWER_SEED)
    n, showsz, radius, background = 700, 96, 3, (40, 90, 160)
    points = (rng.randn(n, 3) * [1.0, 0.7, 0.4]).astype(dtype)
    colours = rng.uniform(0, 255, (n, 3)).astype(np.float32)
    mousex, mousey, zoom = 0.31, 0.68, 1.1
    mod.showsz, mod.mousex, mod.mousey, mod.zoom = showsz, mousex, mousey, zoom
    rec.calls.clear()
    # the viewer normalises its colour argument in place, through views: hand it copies
    mod.showpoints(points.copy(), colours.copy(), None, waittime=1, background=background,
                   normalizecolor=normalizecolor, ballradius=radius)
    assert len(rec.calls) == 1
    c = rec.calls[0]
    assert tuple(c["background"]) == background and (c["h"], c["w"], c["r"]) == (96, 96, radius)
    np.savez_compressed(
        path, points=points, colours=colours, showsz=showsz, ballradius=radius,
        background=np.array(background, np.uint8), normalizecolor=normalizecolor, zoom=zoom,
        mousex=mousex, mousey=mousey, xangle=(mousey - 0.5) * np.pi * 1.2,
        yangle=(mousex - 0.5) * np.pi * 1.2, h=c["h"], w=c["w"], r=c["r"], ixyz=c["ixyz"],
        c0=c["c0"], c1=c["c1"], c2=c["c2"], image=c["image"])
    covered = int((c["image"] != np.array(background, np.uint8)).any(-1).sum())
    print(os.path.basename(path), c["ixyz"].shape, "covered", covered)


def direct(lib, h, w, ixyz, colours, r, background):
    show = np.empty((h, w, 3), np.uint8)
    show[:] = background
    ixyz = np.ascontiguousarray(ixyz, np.int32)
    c = [np.ascontiguousarray(colours[:, k], np.float32) for k in range(3)]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    lib.render_ball(ctypes.c_int(h), ctypes.c_int(w), p(show), ctypes.c_int(len(ixyz)), p(ixyz),
                    p(c[0]), p(c[1]), p(c[2]), ctypes.c_int(r))
    return show


def edge_points():
    h, w = 48, 80
    pts = [(10, 10, 5)] * 5                                   # identical, different colours
    pts += [(20, 20, 7), (20, 22, 7), (21, 21, 7), (19, 21, 7), (20, 21, 4)]  # equal z2 at a pixel
    pts += [(0, 30, 3), (47, 30, 3), (25, 0, 3), (25, 79, 3)]  # the four borders
    pts += [(0, 0, 9), (47, 79, 9), (0, 79, 2), (47, 0, 2)]    # the corners
    pts += [(-2, 40, 6), (49, 44, 6), (30, -3, 6), (33, 82, 6)]  # the centre outside, the disk in
    pts += [(-60, -60, 1), (300, 400, 2), (24, 1000, 3), (-1000, 40, 4)]  # wholly outside
    pts += [(30, 50, -20), (30, 52, -300), (32, 51, -20), (36, 60, -120)]  # negative z
    rng = np.random.RandomState(5)
    rand = np.stack([rng.randint(-5, h + 5, 40), rng.randint(-5, w + 5, 40),
                     rng.randint(-50, 50, 40)], 1)
    ixyz = np.concatenate([np.array(pts, np.int32), rand.astype(np.int32)])
    colours = rng.uniform(0, 255, (len(ixyz), 3)).astype(np.float32)
    colours[1], colours[2] = 255.0, 0.0
    return h, w, ixyz, colours


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    root = sys.argv[1]
    os.makedirs(HERE, exist_ok=True)
    utils = os.path.join(root, "pointnet2_tensorflow", "utils")
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "render_balls_so.so")
        subprocess.run(["g++", "-O2", "-shared", "-fPIC", os.path.join(utils, "render_balls_so.cpp"),
                        "-o", so], check=True)
        lib = ctypes.CDLL(so)
        lib.render_ball.restype = None
        mod, rec = load_viewer(root, lib)
        viewer_case(mod, rec, np.float32, True, os.path.join(HERE, "viewer_f32.npz"))
        viewer_case(mod, rec, np.float64, False, os.path.join(HERE, "viewer_f64.npz"))

        h, w, ixyz, colours = edge_points()
        background = (7, 200, 31)
        out = {"h": h, "w": w, "ixyz": ixyz, "colours": colours,
               "background": np.array(background, np.uint8), "radii": np.array([0, 4, 40])}
        for r in (0, 4, 40):
            out[f"image_r{r}"] = direct(lib, h, w, ixyz, colours, r, background)
        np.savez_compressed(os.path.join(HERE, "direct.npz"), **out)

        one = np.array([[5, 6, -3]], np.int32)
        col = np.array([[200.0, 17.5, 99.0]], np.float32)
        np.savez_compressed(os.path.join(HERE, "n1.npz"), h=12, w=9, r=4, ixyz=one,
                     colours=col, background=np.array((1, 2, 3), np.uint8),
                     image=direct(lib, 12, 9, one, col, 4, (1, 2, 3)))

    # (e) the palette, as data
    path = os.path.join(root, "attention_points", "visualization", "qualitative_animations.py")
    found = {}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name) and \
                node.targets[0].id in ("g_label_names", "g_label_colors"):
            found[node.targets[0].id] = ast.literal_eval(node.value)
    assert len(found["g_label_names"]) == len(found["g_label_colors"]) == 21
    with open(os.path.join(HERE, "palette.json"), "w") as f:
        json.dump({"label_names": found["g_label_names"], "label_colors": found["g_label_colors"]},
                  f, separators=(",", ":"))


if __name__ == "__main__":
    main()
