"""Shared by the training benchmarks (tools/bench_*_train*.py, bench_optim.py): the alternating,
event-timed measurement window, its summary, the peak-allocation probe and the runner that gives
every shape a child process of its own. Not a tool."""
import argparse
import json
import os
import statistics
import subprocess
import sys


def windows(torch, fns, repeats, iters):
    """Per fn the times per call (us) of `repeats` windows of `iters` calls, alternating."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return times


def summary(times):
    return {"us": round(statistics.median(times), 1),
            "min_max_us": [round(min(times), 1), round(max(times), 1)]}


def peak_delta(torch, fn):
    """Bytes one call allocates at its peak above what is held before it."""
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def main(script, shapes, one, iters=10, timeout=120, header=None, options=()):
    """The command line of a benchmark over `shapes`: each shape runs `one(name, repeats, iters)`
    in a child process of its own under `timeout` and prints one JSON line; a shape that fails
    stops the run. --out writes {**header, "shapes": [the lines]} as one JSON file. `options`:
    (flag, add_argument keywords) of the tool's own string options; a given one reaches the
    child's command line and `one` as a keyword (--precision bf16: one(..., precision="bf16"))
    and the header."""
    ap = argparse.ArgumentParser()
    for flag, kw in options:
        ap.add_argument(flag, **kw)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=iters)
    ap.add_argument("--timeout", type=int, default=timeout, help="seconds per shape")
    ap.add_argument("--out", default=None, help="write the results as one JSON file")
    ap.add_argument("--shapes", default=",".join(shapes), help="comma-separated subset")
    ap.add_argument("--one", choices=tuple(shapes), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    extra = {flag.lstrip("-").replace("-", "_"): flag for flag, _ in options}
    given = {k: getattr(args, k) for k in extra if getattr(args, k) is not None}
    if args.one:
        return one(args.one, args.repeats, args.iters, **given)
    results = []
    for name in args.shapes.split(","):
        if name not in shapes:
            ap.error(f"unknown shape {name!r}")
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(script),
               "--one", name, "--repeats", str(args.repeats), "--iters", str(args.iters)]
        for k, v in given.items():
            cmd += [extra[k], str(v)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-2000:])
        if r.returncode != 0:
            sys.exit(f"{name}: exit status {r.returncode}; stopping")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({**(header or {}), **given, "shapes": results}, f, indent=1)
            f.write("\n")
