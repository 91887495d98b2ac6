"""The ball renderer's rule restated in numpy, for test_render_cpu.py and test_gpu_render.py: every
pixel holds the key ((z2 + 2^31) << 32) | (0xFFFFFFFF - i), every (point, disk entry) pair applies
an unsigned max, and a resolve pass shades the winners (include/pn2hip.h, "scene rendering"). Not
a test module."""
import os

import numpy as np


def disk(r):
    """(dx, dy, int(dz), float32(dz / r)) of the entries with dx^2 + dy^2 < r^2, r >= 1."""
    d = np.arange(-r, r + 1)
    dx, dy = [a.ravel() for a in np.meshgrid(d, d, indexing="ij")]
    m = r * r - dx * dx - dy * dy
    keep = m > 0
    dz = np.sqrt(m[keep].astype(np.float64))
    return dx[keep], dy[keep], dz.astype(np.int64), (dz / r).astype(np.float32)


def keys_of(ixyz, r, h, w):
    """(h * w) uint64 keys of one frame, 0 where nothing draws."""
    r = max(int(r), 1)
    p = np.asarray(ixyz, np.int64)
    idx = np.arange(len(p), dtype=np.uint64)
    keys = np.zeros(h * w, np.uint64)
    for dx, dy, idz, _ in zip(*disk(r)):
        x2, y2, z2 = p[:, 0] + dx, p[:, 1] + dy, p[:, 2] + idz
        ok = (x2 >= 0) & (x2 < h) & (y2 >= 0) & (y2 < w) & (z2 > -2100000000)
        key = ((z2[ok] + 2 ** 31).astype(np.uint64) << np.uint64(32)) | \
            (np.uint64(0xFFFFFFFF) - idx[ok])
        np.maximum.at(keys, x2[ok] * w + y2[ok], key)
    return keys


def render_ball(ixyz, c0, c1, c2, r, h, w, background):
    """One frame, (h, w, 3) uint8, in the reference's channel order (c2, c0, c1)."""
    r = max(int(r), 1)
    p = np.asarray(ixyz, np.int64)
    show = np.empty((h * w, 3), np.uint8)
    show[:] = np.asarray(background, np.uint8)
    if len(p) == 0:
        return show.reshape(h, w, 3)
    keys = keys_of(p, r, h, w)
    pix = np.flatnonzero(keys)
    i = (np.uint64(0xFFFFFFFF) - (keys[pix] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    z2 = (keys[pix] >> np.uint64(32)).astype(np.int64) - 2 ** 31
    dx, dy = pix // w - p[i, 0], pix % w - p[i, 1]
    shade = (np.sqrt((r * r - dx * dx - dy * dy).astype(np.float64)) / r).astype(np.float32)
    zmin, zmax = float(p[:, 2].min() - r), float(p[:, 2].max() + r)
    intensity = np.minimum(1.0, (z2.astype(np.float64) - zmin) / (zmax - zmin) * 0.7 + 0.3)
    for k, c in enumerate((c2, c0, c1)):
        c = np.asarray(c, np.float32)[i]
        c = np.where(c >= 0, np.minimum(c, np.float32(255)), np.float32(0)).astype(np.float32)
        show[pix, k] = ((shade * c).astype(np.float64) * intensity).astype(np.int64).astype(np.uint8)
    return show.reshape(h, w, 3)


def project(xyz, mat):
    """One frame's ixyz: (x*R[0][k] + y*R[1][k]) + z*R[2][k] + off[k] in double, truncated."""
    x, y, z = [np.asarray(xyz)[:, k].astype(np.float64) for k in range(3)]
    R, off = np.asarray(mat, np.float64)[:9].reshape(3, 3), np.asarray(mat, np.float64)[9:]
    cols = [(x * R[0, k] + y * R[1, k]) + z * R[2, k] + off[k] for k in range(3)]
    return np.stack(cols, 1).astype(np.int32)


# ------------------------------------------------------------------------------- the goldens
def golden_calls(golden_dir):
    """name -> dict(ixyz (n,3) int32, c (3,n) float32, r, h, w, background, image): every
    render_ball call of tests/golden/render/*.npz (make_golden_render.py), the reference's own
    output."""
    calls = {}
    for name in ("viewer_f32", "viewer_f64"):
        g = np.load(os.path.join(golden_dir, f"{name}.npz"))
        calls[name] = dict(ixyz=g["ixyz"], c=np.stack([g["c0"], g["c1"], g["c2"]]), r=int(g["r"]),
                           h=int(g["h"]), w=int(g["w"]), background=g["background"],
                           image=g["image"])
    g = np.load(os.path.join(golden_dir, "direct.npz"))
    for r in g["radii"]:
        calls[f"direct_r{r}"] = dict(ixyz=g["ixyz"], c=np.ascontiguousarray(g["colours"].T),
                                     r=int(r), h=int(g["h"]), w=int(g["w"]),
                                     background=g["background"], image=g[f"image_r{r}"])
    g = np.load(os.path.join(golden_dir, "n1.npz"))
    calls["n1"] = dict(ixyz=g["ixyz"], c=np.ascontiguousarray(g["colours"].T), r=int(g["r"]),
                       h=int(g["h"]), w=int(g["w"]), background=g["background"], image=g["image"])
    return calls
