"""What the per-call bench tools (tools/<call>_bench.py) share: the paths, the event timer, the
statistics and the ordering gate, graph capture, the sampling loop, and the head and tail of
`main`.  A tool keeps what is about its call (state, exactness checks, variants, the fields of
its result row) and takes its timing and reporting from here; it defines none of its own.

Importing this module needs neither a GPU nor a built library: wtp_crc32 is loaded by `start`
only (a tool that uses the binding itself imports it after this module, which has put its
directory on sys.path)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("a3-reliable-transport_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))


# ---- one timed window, and what is made of its samples ----------------------------------------
def timed(fn, before=None):
    """Milliseconds of `fn()` between two device events; `before()` runs ahead of the window."""
    if before:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(xs):
    a = np.sort(np.asarray(xs, dtype=np.float64))
    return {"median": round(float(np.median(a)), 4), "min": round(float(a[0]), 4), "max": round(float(a[-1]), 4),
            "p25": round(float(np.percentile(a, 25)), 4), "p75": round(float(np.percentile(a, 75)), 4)}


def iqr(xs):
    return float(np.percentile(xs, 75) - np.percentile(xs, 25))


def spread(xs):
    """The interquartile range as a fraction of the median."""
    return round(float(iqr(xs) / np.median(xs)), 4)


def below_by_more_than_both_iqr(xs, ys):
    """The ordering gate: the median of `xs` is below that of `ys` by more than the sum of both
    interquartile ranges (a difference equal to that sum is not below)."""
    return bool(float(np.median(ys)) - float(np.median(xs)) > iqr(xs) + iqr(ys))


# ---- what is timed ----------------------------------------------------------------------------
def graph_of(fn):
    """`fn` once on a side stream (what it leaves behind is the state the graph starts from),
    then captured there."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def repeated(variants, how):
    """Sampling units from {name: (fn, k)}: a unit is k calls of fn in one timed window, replayed
    from a captured graph (`how` == "graph") or issued back to back."""
    units = {}
    for name, (fn, k) in variants.items():
        many = (lambda fn=fn, k=k: [fn() for _ in range(k)])
        units[name] = (graph_of(many).replay if how == "graph" else many, None, k)
    return units


def sample(units, reps, warmup, alternate=False, timer=timed):
    """{name: [ms per unit]} of `reps` repetitions after `warmup` uncounted ones, from
    {name: (run, before, k)}: `run` is timed, `before` (or None) runs ahead of its window, and
    the time is divided by `k`.  A repetition times every unit once: in the order given, or with
    `alternate` in sorted name order on even repetitions (warm-up ones counted) and reversed on
    odd ones."""
    names = sorted(units) if alternate else list(units)
    t = {name: [] for name in names}
    for rep in range(warmup + reps):
        for name in (names[::-1] if alternate and rep % 2 else names):
            run, before, k = units[name]
            ms = timer(run, before) / k
            if rep >= warmup:
                t[name].append(ms)
    return t


# ---- small converters -------------------------------------------------------------------------
def u32(t):
    return t.cpu().numpy().view(np.uint32)


def i32(a):
    """Unsigned 32-bit host values as the int32 device tensor the binding takes."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def z(k, dtype=torch.int32, fill=0):
    return torch.full((k,), fill, dtype=dtype, device="cuda")


# ---- the head and tail of main ----------------------------------------------------------------
def parser():
    """The arguments every tool starts with; the tool adds its own, then `add_out`."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    return ap


def add_out(ap, call):
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", call, call + "_bench.json"))


def result_head(tool, args, device, library, lib_path):
    return {"tool": tool, "device": device, "library": library, "lib_path": lib_path, "reps": args.reps, "warmup": args.warmup}


def start(tool, args, min_reps):
    """Refuses a machine without a GPU and too few repetitions, initialises the library and
    returns the head of the tool's result."""
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: needs a GPU (no CPU fallback)")
    if args.reps < min_reps:
        raise SystemExit(f"{tool}: --reps must be at least {min_reps}")
    import wtp_crc32 as W
    assert W.LIB.wtp_init(0) == 0, W.LIB.wtp_last_error()
    return result_head(tool, args, torch.cuda.get_device_name(0), W.LIB.wtp_version().decode(),
                       os.path.relpath(W.LIB_PATH, ROOT))


def write_result(res, out):
    """The result as one JSON line, written to `out` and printed."""
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)
