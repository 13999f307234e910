"""Ingest-time feature scaling (csrc/ingest.hip) on fp64 frames of the 1M-tet scene's shapes: node frame [1 010 078, 29] with the
loss-weight copy in column 0, edge frame [4 040 312, 20].  Per frame and scaler: device time of ops.scale_features (events, warm-up,
median of the rounds), the bytes its passes must move and their share of 8 TB/s, and the numpy model (tests/ingest_scalers_model.py) on
the host.  `standard` through the new entry point is timed against dgnn_standardize_f64 (data.standardize's call), alternating in
every round.

    python tools/bench_ingest.py [--rounds R] [--iters K] [--no-host] [--split] [--frame node|edge]

--split first runs, per frame, one call per scaler in a child process under `rocprofv3 --kernel-trace --stats` and prints the per-kernel
split of its kernel_stats table with each pass's share of 8 TB/s; if a child fails or runs out of time, the tool ends there.  One JSON line per frame and scaler.

Bytes per element that must move: every statistics pass reads the fp64 frame once (8 B), the apply pass reads it and writes fp32 (12 B):
standard 2 passes + apply = 28 B, minmax 1 + apply = 20 B, robust 8 digit passes + the s[lo+1] pass + apply = 84 B."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--tets", type=int, default=1010078)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--no-host", action="store_true")
ap.add_argument("--split", action="store_true")
ap.add_argument("--split-timeout", type=int, default=300, help="seconds the profiled child of --split may take")
ap.add_argument("--frame", choices=("node", "edge"), help="this frame alone")
ap.add_argument("--once", action="store_true", help="one call per frame and scaler, nothing timed (what --split profiles)")
args = ap.parse_args()

BYTES = {"standard": 28, "minmax": 20, "robust": 84}
PEAK = 8e12


SHAPES = (("node", args.tets, 29, 1), ("edge", 4 * args.tets, 20, 0))


def frames(only=None):
    out = {}
    for i, (name, n, c, c_first) in enumerate(SHAPES):
        if only not in (None, name):
            continue
        rng = np.random.default_rng(i)
        x = np.empty((n, c))
        for j in range(c):          # the real frames' mix: heavy-tailed geometry, small counts with ties, distances that are 0 where the count is
            cnt = rng.poisson(3, n).astype(np.float64)
            x[:, j] = (rng.lognormal(0, 1.5, n), cnt, rng.exponential(5.0, n) * (cnt > 0), rng.exponential(20.0, n) * cnt)[j % 4]
        out[name] = (x, c_first)
    return out


# bytes per element a kernel's one call must move: a statistics pass reads the fp64 frame, the apply reads it and writes fp32
PASS_BYTES = {"k_sc_colreduce<0>": 8, "k_sc_colreduce<1>": 8, "k_sc_extrema": 8, "k_sc_hist": 8, "k_sc_next": 8, "k_sc_apply": 12}

if args.split:
    for name, n, c, _ in SHAPES:          # one child per frame, so a kernel's calls all walk the same bytes
        d = tempfile.mkdtemp(prefix="ingest_split_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "split", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--once", "--frame", name, "--tets", str(args.tets)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.split_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("the profiled child did not finish in %d s: nothing more is started on the device" % args.split_timeout)
        if r.returncode:          # a fault, an abort or a kill in the child: this process does not open the device after it
            sys.exit("the profiled child ended with status %d: nothing more is started on the device\n%s" % (r.returncode, r.stderr[-800:]))
        tables = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not tables:
            print("per-kernel split unavailable (no kernel_stats table among %s)" % glob.glob(os.path.join(d, "**", "*"), recursive=True)[:8])
            continue
        print("per-kernel split, %s frame [%d, %d], one call per scaler (rocprofv3 kernel_stats):" % (name, n, c))
        print("  %-20s %5s %10s %10s %10s  %s" % ("kernel", "calls", "mean us", "min us", "max us", "share of 8 TB/s at the mean (B / element / call)"))
        for row in csv.DictReader(open(tables[0])):
            k = re.search(r"k_(?:sc|ing)_\w+(?:<\d>)?", row["Name"])
            if not k:
                continue
            avg = float(row["AverageNs"])
            b = PASS_BYTES.get(k.group(0))
            share = "%5.1f %%  (%d)" % (100 * n * c * b / (avg * 1e-9) / PEAK, b) if b else "no pass over the frame"
            print("  %-20s %5s %10.1f %10.1f %10.1f  %s" % (k.group(0), row["Calls"], avg / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3, share))
        sys.stdout.flush()

from dgnn_amd import ops  # noqa: E402
from dgnn_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402

dev = "cuda:0"
fr = frames(args.frame)

if args.once:
    for name, (x, c_first) in fr.items():
        xd = torch.from_numpy(x).to(dev)
        for kind in BYTES:
            ops.scale_features(xd, c_first, kind)
    torch.cuda.synchronize()
    sys.exit(0)

import ingest_scalers_model as M  # noqa: E402


def timed(f, it=args.iters, warm=3):
    for _ in range(warm):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(it):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / it


for name, (x, c_first) in fr.items():
    xd = torch.from_numpy(x).to(dev)
    n, c = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    scratch = torch.empty(int(lib().dgnn_standardize_scratch_doubles(c)), dtype=torch.float64, device=dev)

    def old():
        check(lib().dgnn_standardize_f64(ptr(xd), c, n, c, c_first, ptr(out), c, ptr(scratch), stream_ptr()), "dgnn_standardize_f64")

    t = {k: [] for k in ("old_standard", "standard", "minmax", "robust")}
    for _ in range(args.rounds):          # the paths alternate inside every round: all see the same clocks
        t["old_standard"].append(timed(old))
        for kind in BYTES:
            t[kind].append(timed(lambda: ops.scale_features(xd, c_first, kind)))
    host = {}
    if not args.no_host:
        for kind in BYTES:
            t0 = time.perf_counter()
            M.scale_frame(x, c_first, kind)
            host[kind] = (time.perf_counter() - t0) * 1e3
    for kind in BYTES:
        ms = statistics.median(t[kind])
        rec = {"frame": name, "rows": n, "cols": c, "kind": kind, "device_ms": round(ms, 4), "device_ms_min_max": [round(min(t[kind]), 4), round(max(t[kind]), 4)],
               "bytes_per_element": BYTES[kind], "GBps": round(n * c * BYTES[kind] / ms / 1e6, 1),
               "share_of_8TBps": round(n * c * BYTES[kind] / (ms * 1e-3) / PEAK, 3)}
        if kind == "standard":
            o = statistics.median(t["old_standard"])
            rec.update(dgnn_standardize_f64_ms=round(o, 4), new_over_old=round(ms / o, 3))
        if host:
            rec.update(host_numpy_ms=round(host[kind], 1), host_over_device=round(host[kind] / ms, 1))
        print(json.dumps(rec), flush=True)
