#!/usr/bin/env python3
"""Benchmark of the ball renderer (csrc/render.hip) on a synthetic room (synth.scannet_scene,
200,000 points) coloured by label, 800 x 800, radius 10, the reference viewer's defaults: one
frame and an orbit of 120 frames through show3d_balls.render (projection, splat, resolve; the
orbit in chunks of MAX_CHUNK_BYTES), event-timed windows after a warm-up, each of --iters
orbits or as many single frames, medians (tools/_timing.py). Beside them the passes on their
own (the projection; the renderer on projected points; the renderer with no points, which is
its memset and a resolve that only writes the background) and the host twin's time for one such frame (pn2cpu_render_ball, one
core), which does the work of the reference's serial loop.

Variants of the splat, each a build of its own loaded in a child process:
  skip    the product: read the key, skip the atomic when it is already >= the candidate
  plain   one 64-bit atomic max per (point, disk entry):
          make -C pointcloud-segmentation-attention_amd/csrc abdir VNAME=render_plain \\
               VFLAGS=-DPN2_RENDER_SKIP=0
A variant whose build is missing is reported as such, not measured.

--out writes profiles/render/summary.json."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _timing  # noqa: E402

PKG = "pointcloud-segmentation-attention_amd"
N_POINTS, SIZE, RADIUS, ORBIT = 200000, 800, 10, 120
VARIANTS = {"skip": None,
            "plain": os.path.join(ROOT, PKG, "csrc", "build", "ab_render_plain")}
SHAPES = ("frames_1", "frames_120", "host_twin")


def scene(pkg):
    import numpy as np
    points, labels, _, _ = pkg.synth.scannet_scene(7, N_POINTS)
    palette = np.random.default_rng(1).uniform(30, 255, (21, 3)).astype(np.float32)
    palette[0] = 0
    return points, labels, palette


def one(name, repeats, iters):
    import numpy as np
    import torch
    pkg = importlib.import_module(PKG)
    s, v = pkg.show3d_balls, pkg.visualization
    points, labels, palette = scene(pkg)
    xyz_host = s.prepare(points, SIZE)
    res = {"shape": name, "points": N_POINTS, "size": [SIZE, SIZE], "radius": RADIUS}
    if name == "host_twin":
        xa, ya = v.orbit(ORBIT)[7]
        mats = s.view_matrices(xa, ya, 1.0, SIZE, SIZE)
        xyz, lab, pal = torch.from_numpy(xyz_host), torch.from_numpy(labels), torch.from_numpy(palette)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            s.render(xyz, mats, SIZE, SIZE, RADIUS, v.WHITE, labels=lab, palette=pal)
            times.append((time.perf_counter() - t0) * 1e6)
        res.update(frames=1, per_frame=_timing.summary(times), what="wall clock of 3 calls")
        print(json.dumps(res), flush=True)
        return
    assert torch.cuda.is_available(), "bench_render.py measures on the MI355X only"
    dev = torch.device("cuda:0")
    F = int(name.split("_")[1])
    iters *= ORBIT // F  # every window renders as many frames as the orbit's does
    xa, ya = zip(*v.orbit(ORBIT)[:F]) if F > 1 else ([np.pi / 4], [0.6])
    mats = s.view_matrices(xa, ya, 1.0, SIZE, SIZE)
    xyz, lab, pal = (torch.from_numpy(a).to(dev) for a in (xyz_host, labels, palette))
    ops = importlib.import_module(PKG + "._torch_ops").ops()
    # the passes on one chunk of frames (the orbit's first chunk)
    per_frame = 8 * SIZE * SIZE + 12 * N_POINTS + 1
    chunk = int(max(1, min(F, s.MAX_CHUNK_BYTES // per_frame)))
    m = torch.from_numpy(mats[:chunk]).to(dev)
    ixyz = ops.render_project(xyz, m)
    none = torch.zeros(chunk, 0, 3, dtype=torch.int32, device=dev)
    nolab = torch.zeros(0, dtype=torch.int32, device=dev)
    bg = list(v.WHITE)
    fns = [lambda: s.render(xyz, mats, SIZE, SIZE, RADIUS, v.WHITE, labels=lab, palette=pal),
           lambda: ops.render_project(xyz, m),
           lambda: ops.render_ball(ixyz, None, None, None, lab, pal, RADIUS, SIZE, SIZE, bg),
           lambda: ops.render_ball(none, None, None, None, nolab, pal, RADIUS, SIZE, SIZE, bg)]
    whole, project, ball, empty = _timing.windows(torch, fns, repeats, iters)
    covered = int((fns[0]()[0] != 255).any(-1).sum())
    res.update(frames=F, chunk_frames=chunk, covered_pixels_frame0=covered,
               per_frame=_timing.summary([t / F for t in whole]),
               project_per_frame=_timing.summary([t / chunk for t in project]),
               ball_per_frame=_timing.summary([t / chunk for t in ball]),
               memset_and_empty_resolve_per_frame=_timing.summary([t / chunk for t in empty]))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default=None, help="write the results as one JSON file")
    ap.add_argument("--one", choices=SHAPES, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.repeats, args.iters)
    results = []
    for variant, build in VARIANTS.items():
        env = dict(os.environ)
        if build is not None:
            libs = [os.path.join(build, n) for n in ("libpn2hip.so", "libpn2torch.so")]
            if not all(os.path.exists(p) for p in libs):
                results.append({"variant": variant, "skipped": "its build is missing"})
                print(json.dumps(results[-1]), flush=True)
                continue
            env["PN2HIP_LIB"], env["PN2TORCH_LIB"] = libs
        for name in SHAPES:
            if name == "host_twin" and build is not None:
                continue  # the twin has no variants
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable,
                   os.path.abspath(__file__), "--one", name, "--repeats", str(args.repeats),
                   "--iters", str(args.iters)]
            r = subprocess.run(cmd, capture_output=True, text=True, env=env)
            sys.stderr.write(r.stderr[-2000:])
            if r.returncode != 0:
                sys.exit(f"{variant} {name}: exit status {r.returncode}; stopping")
            line = {"variant": variant, **json.loads(r.stdout.strip().splitlines()[-1])}
            print(json.dumps(line), flush=True)
            results.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"what": "us per frame, median of the windows (min, max beside it); "
                               "synth.scannet_scene(7, 200000) by label, 800 x 800, radius 10",
                       "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
