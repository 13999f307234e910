#!/usr/bin/env python3
"""Benchmark of the dgnn hot path on MI355X: whole-graph in/out classification of a synthetic Delaunay
tetrahedron graph (SurfaceNet.inference_layer equivalent: 4 x [edge-filtered SAGE conv + BN(eval) +
ReLU] + decoder -> logits [N,2]), shipped kf96 weights.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over the graph, inputs resident in HBM in the reference's layout
(x [N,29] fp32, edge_attr [4N,20] fp32, edge_index [2,4N] int64).  The step INCLUDES building the
graph plan (stable destination sort), because the reference takes a raw edge_index on every call.
N>1: the scene is partitioned spatially, one part per rank; every part keeps the rings of cells 1..4 hops outside it resident and recomputes each
layer on the rings later layers still read (`--halo recompute`, default: no collective in the data path, one library call per step; a ring of a
1/8 part of the 1M-tet scene is 3.7 % of its cells) -- or, `--halo exchange`, keeps one ring and exchanges its rows over RCCL before conv layers
1..3 (the form the partitioned backward uses).  `--scaling strong` (default since round 4: the metric's "1M-tet graph at 1/2/4/8"): the `--points` scene
itself cut N ways; `--scaling weak`: gpus x `--points` points, ~1M tets per GPU (nested under `other_scaling`).  Rank 0 prints ONE JSON line.

Secondary lines: `--widths 64,128,256,512`, `--widths 128,256,512,1024` (random-init weights,
torch.manual_seed(0)), `--points 1485000` (10M tets), `--dtype bf16` (bf16 storage + single-product bf16 MFMA).

After the timed steps the run CHECKS itself: the CPU oracle (the timed CPU baseline, same graph, same weights) and the
GPU logits are compared (`check`), and the process exits non-zero when they differ by more than the stated tolerance.

`--dump-outputs DIR` writes what the last timed step returned as .npy files (see the option's help).  Inputs are seeded, so two builds
run with the same arguments can be compared output for output.
"""
from __future__ import annotations

import argparse
import shutil
import glob
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0         # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
TOL_F32 = 1e-4                # |dlogit| <= TOL * max(1, |logit|)  (tests/test_gpu_scale.py header)
TOL_BF16 = 5e-2               # bf16 storage path, arg-max agreement >= 99.9 %


def layer_bytes(c_in, c_out, elem=4):
    """algorithmic HBM bytes per tet of one fused conv layer: x read once (own row), 4 edge rows of 20 fp32,
    4 int32 source ids, out written once.  `elem` = bytes per activation element (4 fp32, 2 bf16 storage)."""
    return elem * c_in + 320 + 16 + elem * c_out


def layer_flops(c_in, c_out):
    """algorithmic FLOPs per tet of one conv layer: lin_e on 4 edges, the 4-term product-sum, lin_j + lin_i."""
    return 4 * 2 * 20 * c_in + 8 * c_in + 4 * c_in * c_out


FP32_MATRIX_PEAK_TF = 157.3   # MI355X_MICROARCH.md: fp32-input MFMA peak (= the fp32 vector peak)
BF16_MATRIX_PEAK_TF = 2500.0  # dense bf16 MFMA peak


def path_bytes(f_in, widths, elem=4):
    """whole path: conv layers + decoder (reads the last activations, writes 2 fp32 logits): 5048 B/tet for the shipped widths."""
    cs = [f_in] + list(widths)
    return sum(layer_bytes(a, b, elem) for a, b in zip(cs[:-1], cs[1:])) + elem * widths[-1] + 8


def wide_layer_is_split_rows(net, c_in, c_out):
    """True when the model runs the c_in -> c_out conv layer on the split-row kernels (round 5: csrc/wide.hip)"""
    fn = getattr(net, "wide_layer_split_rows", None)
    return bool(fn(c_in, c_out)) if fn is not None else False


def load_weights():
    w = np.load(os.path.join(ROOT, "tests", "golden", "kf96_weights.npz"))
    return {k: torch.from_numpy(w[k]) for k in w.files}


def make_scene(points, seed):
    from dgnn_amd.synthetic import delaunay_tet_graph
    adj, cent, _ = delaunay_tet_graph(points, seed)
    n = adj.shape[0] // 4
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, 29, generator=g)
    ea = torch.randn(4 * n, 20, generator=g)
    return adj, cent, x, ea


def csrc_sha():
    """Hash of the fused layer kernels' sources: the PMC-derived fields of `roofline` are only valid for the kernels they were
    measured on (profiles/*_traffic.json carries the hash of the sources it profiled)."""
    h = hashlib.sha256()
    # the sources the profiled launches are compiled from: the fused layer kernels (fp32 / bf16 storage) and the headers they include
    for p in sorted(glob.glob(os.path.join(ROOT, "dgnn_amd", "csrc", "fused*.hip")) + [os.path.join(ROOT, "dgnn_amd", "csrc", h) for h in ("common.h", "fused_common.h")]):
        h.update(os.path.basename(p).encode())
        h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def cpu_oracle(net_sd, convs, x, ea, ei, threads, runs):
    """Times the CPU oracle (plain-PyTorch restatement of the reference path; test infrastructure, used here only as the
    timed CPU baseline and as the checker).  -> (median seconds, logits).  runs = -1: ONE call, timed as it is (no warm-up)."""
    from dgnn_amd.config import Config, reconbench_pretrained
    from oracle.static_edge_filters import SurfaceNet as OracleNet
    net = OracleNet(reconbench_pretrained(device="cpu", convs=convs))
    net.load_state_dict(net_sd)
    net.eval()
    data = Config(x=x, edge_attr=ea, edge_index=ei)
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    times = []
    with torch.no_grad():
        t0 = time.perf_counter()
        out = net.inference_layer(data)                 # warm-up (also the checker's reference logits)
        if runs < 0:
            times.append(time.perf_counter() - t0)
        for _ in range(runs):
            t0 = time.perf_counter()
            net.inference_layer(data)
            times.append(time.perf_counter() - t0)
    torch.set_num_threads(old)
    return (float(np.median(times)) if times else float("nan")), out


def gpu_state_sample():
    """one reading of shader clock (MHz) and package power (W) of the current GPU through rocm-smi, or None"""
    import re
    import subprocess
    try:
        o = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=10).stdout
        dev = os.environ.get("LOCAL_RANK", "0")
        clk = [re.search(r"\((\d+)Mhz\)", l) for l in o.splitlines() if "sclk" in l and ("GPU[%s]" % dev) in l]
        pw = [re.search(r":\s*([\d.]+)\s*$", l) for l in o.splitlines() if "Power (W)" in l and ("GPU[%s]" % dev) in l]
        return (int(clk[0].group(1)) if clk and clk[0] else None, float(pw[0].group(1)) if pw and pw[0] else None)
    except Exception:  # noqa: BLE001
        return None


def load_probe(step, seconds=1.5):
    """The timed region lasts tens of milliseconds -- too short for any sensor.  Right after it the same step runs back to back for
    `seconds` while a thread reads shader clock and package power: a box that runs these kernels throttled (about one
    in four did in round 2, at half speed) shows here as a low clock and as probe steps far from the timed ones."""
    import threading
    samples, stop = [], [False]

    def sampler():
        while not stop[0]:
            r = gpu_state_sample()
            if r is not None:
                samples.append(r)
    th = threading.Thread(target=sampler, daemon=True)
    torch.cuda.synchronize()
    th.start()
    t0 = time.perf_counter()
    k = 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        k += 10
    dt = time.perf_counter() - t0
    stop[0] = True
    th.join(timeout=15)
    clk = [c for c, _ in samples[1:] if c] or [c for c, _ in samples if c]
    pw = [p_ for _, p_ in samples[1:] if p_] or [p_ for _, p_ in samples if p_]
    return {"probe_ms_per_step": round(dt / k * 1e3, 4), "probe_steps": k, "sclk_mhz": clk[:8], "power_w": pw[:8],
            "source": "rocm-smi sampled by a thread while the step ran back to back for %.1f s right after the timed region" % seconds}


def timed_steps(step, steps, sync, world, dev, keep=None):
    """EXACTLY `steps` steps between barrier + synchronize on both sides (wall clock, max over ranks) and, from events recorded on the
    launch stream between the steps, the per-step times.  -> (seconds, [ms per step]).  `keep` (a dict): keep["out"] = what the last step returned."""
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    sync()
    t0 = time.perf_counter()
    for i in range(steps):
        evs[i].record()
        if keep is None:
            step()
        else:
            keep["out"] = step()
    evs[steps].record()
    sync()
    dt = time.perf_counter() - t0
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    per = [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]
    if os.environ.get("DGNN_BENCH_DEBUG_STEPS"):
        sys.stderr.write("timed_steps: wall %.3f ms; per step (events) %s\n" % (dt * 1e3, " ".join("%.2f" % v for v in per)))
    return dt, per


DUMP_BUDGET_BYTES = 64 << 20   # --dump-outputs: at most this much on disk per run
DUMP_SAMPLE_SEED = 0


def dump_output(out_dir, name, t, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: tensor `t` (one row per cell) as out_dir/<name>.npy, float64 kept, anything else as float32.  Larger than `budget`:
    a fixed seeded sample of its rows in ascending order, and out_dir/<name>_rows.npy (float64) names them.  -> rows written"""
    a = t.detach().cpu()
    a = (a.double() if a.dtype == torch.float64 else a.float()).numpy()
    os.makedirs(out_dir, exist_ok=True)
    room = budget - 2 * 1024          # (an .npy header takes 128 bytes; two files when sampled)
    if a.nbytes > room:
        # a sampled row costs its values plus its float64 row number
        k = int(room // (a.nbytes // a.shape[0] + 8))
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(a.shape[0], k, replace=False))
        np.save(os.path.join(out_dir, name + "_rows.npy"), rows.astype(np.float64))
        a = a[rows]
    np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))
    return a.shape[0]


def logits_check(got, ref, bf16, bf16_compensated=True):
    """GPU logits against the oracle's on the same graph: the stated tolerance (tests/test_gpu_scale.py, tests/test_gpu_bf16.py)"""
    refn = ref.double()
    err = (got.double() - refn).abs()
    agree = float((got.argmax(1) == ref.argmax(1)).double().mean())
    if bf16:
        # stated tolerance of the bf16 storage path (tests/test_gpu_bf16.py): 5e-2 * max(1, |logit|/8) for >= 99.99 % of the
        # logits and twice that for every one (single-product mode: both doubled), arg-max agreement >= 99.9 % (99.8 %)
        k = 1.0 if bf16_compensated else 2.0
        tol = k * TOL_BF16 * (refn.abs() / 8).clamp_min(1.0)
        inside = float((err <= tol).double().mean())
        margin = (refn[:, 0] - refn[:, 1]).abs() > 2 * tol.max(dim=1).values
        flips_margin = int((got.argmax(1)[margin] != ref.argmax(1)[margin]).sum())
        ok = inside >= 0.9999 and bool((err <= 2 * tol).all()) and flips_margin == 0 and agree >= (0.999 if k == 1.0 else 0.998)
        tol_text = "%g * max(1,|logit|/8) for >= 99.99 %% of the logits (within: %.6f), 2x that for all; arg-max agreement >= %s" % (
            k * TOL_BF16, inside, "99.9 %" if k == 1.0 else "99.8 %")
    else:
        tol = TOL_F32 * refn.abs().clamp_min(1.0)
        margin = (refn[:, 0] - refn[:, 1]).abs() > 2 * tol.max(dim=1).values
        flips_margin = int((got.argmax(1)[margin] != ref.argmax(1)[margin]).sum())
        ok = bool((err <= tol).all()) and flips_margin == 0
        tol_text = "%g * max(1,|logit|)" % TOL_F32
    return {"max_abs_err": float(err.max()), "rms_err": float((err ** 2).mean().sqrt()), "tolerance": tol_text,
            "argmax_flips": int((got.argmax(1) != ref.argmax(1)).sum()), "argmax_flips_above_margin": flips_margin,
            "argmax_agreement": round(agree, 6), "ok": ok}


def relabelled_scene(adj, x, ea, seed=7):
    """the same graph with its cells renumbered at random (what a CGAL-ordered real scene looks like to the gathers: neighbour ids tens of
    thousands of rows apart, tests/golden static_f4): reference layout kept (4 rows per cell, source-major), features move with their cell / edge"""
    n = adj.shape[0] // 4
    perm = np.random.default_rng(seed).permutation(n)          # new id of old cell i
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)                                    # old id of new cell k
    rows = (inv[:, None] * 4 + np.arange(4)[None]).reshape(-1)  # old edge row of new edge row
    adj2 = np.empty_like(adj)
    adj2[:, 0] = np.repeat(np.arange(n, dtype=adj.dtype), 4)
    adj2[:, 1] = perm[adj[rows, 1]]
    return adj2, x[torch.from_numpy(inv)], ea[torch.from_numpy(rows)]


def headline_of(full, full_path):
    """The ONE line the driver reads, kept under 4 KB (the nested legs had pushed it past 15 KB and the driver's tail truncated it): the
    contract's keys whole, `roofline` / `cpu_baseline` / `check` without their prose, one or two numbers per nested leg.  Everything else -- every note, the
    per-launch tables, the side measurements -- is the full object, written to `full_path` (gpurun_out/bench_full.json)."""
    def pick(d, keys):
        return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None} if isinstance(d, dict) else None
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_median", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    h = {k: full[k] for k in keep if k in full}
    cfg = full.get("config") or {}
    h["config"] = pick(cfg, ("workload", "tets_per_gpu", "weights", "plan_in_step", "algorithmic_bytes_per_tet", "decoder"))
    roof = full.get("roofline")
    if roof:
        r = pick(roof, ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "ms", "launches_timed", "algorithmic_bytes_per_launch", "frac_fused",
                        "traffic_over_algorithmic", "whole_path_frac", "matches_this_build"))
        if isinstance(roof.get("also"), dict):
            r["also"] = pick(roof["also"], ("kernel", "achieved", "frac", "ms", "traffic"))
        h["roofline"] = r
    else:
        h["roofline"] = None
    cpu = full.get("cpu_baseline")
    h["cpu_baseline"] = pick(cpu, ("value", "unit", "cores", "kind", "sample", "single_thread_value", "all_cores_value", "all_cores")) if cpu else None
    chk = full.get("check")
    h["check"] = pick(chk, ("ok", "max_abs_err", "rms_err", "tolerance", "argmax_flips", "argmax_flips_above_margin", "argmax_agreement", "bit_identical_to_single_rank",
                            "cells_covered", "n_tets")) if chk else None
    x = full.get("exact_f32")
    if x:
        h["exact_f32"] = {"value": x.get("value"), "ms_per_step": x.get("ms_per_step"), "frac": (x.get("roofline") or {}).get("frac"), "ok": (x.get("check") or {}).get("ok")}
    for k in ("generator_order", "random_cell_order"):
        if full.get(k):
            h[k] = {"value": full[k].get("value")}
    ro = full.get("real_order")
    if ro:
        h["real_order"] = {k: ro[k].get("value") for k in ("morton", "bfs") if isinstance(ro.get(k), dict)}
    b = full.get("bf16_storage")
    if b:
        cb = b.get("check") or {}
        h["bf16_storage"] = {"value": b.get("value"), "ms_per_step": b.get("ms_per_step"), "ok": cb.get("ok"), "max_abs_err": cb.get("max_abs_err"),
                             "argmax_agreement": cb.get("argmax_agreement"), "whole_path_frac": (b.get("roofline") or {}).get("whole_path_frac")}
    w = full.get("wide_widths")
    if w:
        h["wide_widths"] = {k: {"value": v.get("value"), "ms_per_step": v.get("ms_per_step"), "ok": (v.get("check") or {}).get("ok"),
                                "max_abs_err": (v.get("check") or {}).get("max_abs_err")} for k, v in w.items()}
    ss = full.get("small_scenes")
    if ss:
        h["small_scenes"] = pick(ss, ("one_call_ms_per_scene", "one_call_value", "block_diagonal_batch_value"))
    sp = (full.get("strong_scaling_parts") or {}).get("parts")
    if sp:
        h["strong_scaling_parts"] = {k: {"ms": v.get("ms_per_step_rank_first_last"), "same_bits": v.get("bit_identical_to_whole_scene")} for k, v in sp.items()}
    t10 = full.get("scene_10m")
    if t10:
        h["scene_10m"] = pick(t10, ("value", "ms_per_step", "n_tets", "skipped"))
    for k in ("training_step", "training_step_updated_bf16", "training_step_modelnet_widths", "training_step_updated_bf16_modelnet_widths"):
        t = full.get(k)
        if isinstance(t, dict):
            h[k] = pick(t, ("ms_per_step", "targets_per_s", "launches_per_step", "error"))
    cv = full.get("config3_convergence")
    if cv:
        h["config3_convergence"] = pick(cv, ("ok", "steps", "loss_f32_first", "loss_f32_last", "loss_bf16_last", "max_rel_gap_early", "max_rel_gap_late", "band", "error"))
    o = full.get("other_scaling")
    if o:
        h["other_scaling"] = {"scaling": o.get("scaling"), "value": o.get("value"), "ms_per_step": o.get("ms_per_step"), "ok": (o.get("check") or {}).get("ok")}
    for k in ("halo_exchange", "config4_10m"):
        l = full.get(k)
        if l:
            h[k] = {"value": l.get("value"), "ms_per_step": l.get("ms_per_step"), "n_tets": l.get("n_tets"), "rccl_world": l.get("rccl_world"),
                    "transport": (l.get("transport") or "")[:48], "ok": (l.get("check") or {}).get("ok")}
    gs = full.get("gpu_state")
    if isinstance(gs, dict):
        h["gpu_state"] = pick(gs, ("sclk_mhz_under_load", "power_w_under_load", "sclk_mhz", "power_w"))
    h["full"] = full_path
    return h


def write_full(full):
    """the whole nested object -> gpurun_out/bench_full.json (merged back from the GPU box with the rest of gpurun_out/); returns the path it names in the line"""
    rel = os.path.join("gpurun_out", "bench_full.json")
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, rel), "w") as f:
            json.dump(full, f, indent=1)
        tag = os.environ.get("DGNN_BENCH_TAG")
        if tag:
            with open(os.path.join(ROOT, "gpurun_out", "bench_full_%s.json" % tag), "w") as f:
                json.dump(full, f, indent=1)
    except OSError as e:
        sys.stderr.write("bench: could not write %s (%s)\n" % (rel, e))
        return None
    return rel


def start_scene_builder(points, seed):
    """A CPU-only child process (never touches the GPU; started before this process does) that builds the `points`-point Delaunay scene and leaves
    adjacency + centroids as .npy files in a scratch directory: (Popen, directory)."""
    import subprocess
    import tempfile
    d = tempfile.mkdtemp(prefix="dgnn_scene10m_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    code = ("import sys, os, numpy as np; sys.path.insert(0, %r); "
            "from dgnn_amd.synthetic import delaunay_tet_graph; "
            "adj, cent, _ = delaunay_tet_graph(%d, %d); "
            "np.save(os.path.join(%r, 'adj.npy'), np.ascontiguousarray(adj.astype(np.int32))); "
            "np.save(os.path.join(%r, 'cent.npy'), np.ascontiguousarray(cent.astype(np.float32))); "
            "open(os.path.join(%r, 'done'), 'w').close()" % (ROOT, points, seed, d, d, d))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", OMP_NUM_THREADS="4")
    try:
        return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL), d
    except OSError:
        shutil.rmtree(d, ignore_errors=True)
        return None


def drop_scene_builder(h):
    """stops the child (if it still runs) and removes its scratch directory; safe to call twice"""
    if h is None:
        return
    proc, d = h
    if proc.poll() is None:
        proc.kill()          # the exact child started above
        proc.wait()
    shutil.rmtree(d, ignore_errors=True)


def convergence_leg():
    """tools/config3_convergence.py as a child process: both loss curves, the gaps between them and the stated band"""
    import subprocess
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    band = {"early": 0.30, "late": 0.10}       # tests/test_gpu_config3.py: BAND_EARLY (steps < 100), BAND_LATE
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "config3_convergence.py")], capture_output=True, text=True, timeout=120)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": "config3_convergence exited %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or "")}
        d = json.loads(line[-1])
        d["band"] = band
        d["ok"] = bool(d["finite"] and d["max_rel_gap_early"] <= band["early"] and d["max_rel_gap_late"] <= band["late"] and d["loss_bf16_last"] <= 0.05 * d["loss_f32_first"])
        return d
    except Exception as e:  # noqa: BLE001
        return {"error": repr(e)}


def training_leg(extra=()):
    """SURVEY 8d "fwd+bwd+Adam, reported separately": tools/bench_train.py (block builder + SurfaceNet.forward in train mode + KL loss +
    backward + Adam on 2048-target 4-hop blocks of the same scene) run as a child process once the timed inference region is over;
    returns its JSON line (ms_per_step, targets/s, its own roofline object) or the reason it could not run."""
    import subprocess
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    cmd = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "bench_train.py"), "--steps", "200", "--warmup", "300"] + list(extra)
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": "bench_train exited %d: %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or "")}
        return json.loads(line[-1])
    except Exception as e:  # a missing leg must not cost the inference line
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--points", type=int, default=150000, help="Delaunay points (150000 -> 1 010 078 tets; 1485000 -> 10M tets)")
    ap.add_argument("--events-every", type=int, default=4,
                    help="N=1: every k-th timed step carries the per-launch HIP events of the roofline object (the events and the per-layer calls they need cost "
                         "the step 1-2 %%); 1 = every step")
    ap.add_argument("--halo", choices=["recompute", "exchange"], default="recompute",
                    help="N>1: recompute (default) = every part keeps L rings of halo cells and recomputes each layer on the rings later layers read, no collective "
                         "in the data path; exchange = one ring, rows exchanged between the layers over RCCL (the form the partitioned backward uses)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="N>1: strong (default: the metric reads \"1M-tet graph at 1/2/4/8 MI355X\") = the --points scene cut N ways, weak = gpus x --points "
                         "points (fixed work per GPU); the other one is measured too and nested under `other_scaling`")
    ap.add_argument("--widths", type=str, default=None, help="conv widths, e.g. 64,128,256,512 (random-init weights); default: kf96 checkpoint")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default="f32", help="bf16: bf16 activation storage, single-product bf16 MFMA, fp32 accumulate")
    ap.add_argument("--cpu-points", type=int, default=30000, help="sample size of the single-thread CPU leg")
    ap.add_argument("--cell-order", choices=["loader", "generator"], default="loader",
                    help="loader (default): the scene goes through the package's ingest-time cell order first, as every scene read by dgnn_amd.processing.data does; "
                         "generator: cells as generated (the headline of rounds 1-3, nested as `generator_order` otherwise)")
    ap.add_argument("--small-points", type=int, default=10000, help="points of the reconbench-size scenes of the `small_scenes` side measurement (10000 -> ~66k tets)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU oracle legs (and with them the logit check)")
    ap.add_argument("--no-breakdown", action="store_true", help="skip the per-layer replays (the roofline is then reported for the largest layer shape)")
    ap.add_argument("--cached-plan", action="store_true", help="reuse the graph plan across steps (reported, not the metric)")
    ap.add_argument("--no-train", action="store_true", help="skip the training-step leg (tools/bench_train.py as a child process after the "
                                                            "timed region; its line is nested under `training_step`)")
    ap.add_argument("--no-extras", action="store_true", help="skip the nested side measurements (exact-fp32 arithmetic, randomly relabelled graph, clock / power "
                                                             "probe, the other scaling mode at N > 1)")
    ap.add_argument("--scene-10m", choices=["auto", "on", "off"], default="auto",
                    help="N=1 default run: the 10 026 136-tet scene (--points 1485000) as a nested leg `scene_10m`.  Its Delaunay triangulation takes the host about a "
                         "minute, so a child process (CPU only) builds it while the rest of the line is measured; auto = run the leg only if the scene is ready and "
                         "the whole run stays under ~150 s, on = wait for it, off = skip")
    ap.add_argument("--gemm-mode", choices=["f32", "bf16x3", "bf16x3f", "f16x2d", "f16x2"], default=None,
                    help="dense part of the fused fp32 layer: exact fp32 MFMA, or 3-way split-bf16 MFMA (fp32-class accuracy)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the logits, in the cell order the step ran on) as DIR/logits.npy "
                         "(N > 1: DIR/logits_rank<r>.npy, each rank its own cells), float32, at most 64 MB in all: a larger output keeps a fixed seeded "
                         "sample of its rows and names them in DIR/<name>_rows.npy")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")

    t_bench0 = time.perf_counter()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    scene10 = None
    if (world == 1 and args.scene_10m != "off" and not args.no_extras and args.points == 150000 and args.widths is None and args.dtype == "f32"
            and args.gemm_mode is None):
        scene10 = start_scene_builder(1485000, 0)
        if scene10 is not None:
            import atexit
            atexit.register(drop_scene_builder, scene10)      # (a run that ends before the leg -- an exception, sys.exit -- must not leave the child or its files behind)
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run --nproc-per-node %d" % (args.gpus, world, args.gpus))
    # DGNN_BENCH_BACKEND=gloo: validation runs of the multi-rank path on a box with fewer GPUs than ranks (ranks share
    # devices, halo rows are staged through host memory).  The numbers of such a run are not a benchmark.
    backend = os.environ.get("DGNN_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = "cuda:%d" % local_rank
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(dev))
        else:
            dist.init_process_group(backend)

    from dgnn_amd import ops
    from dgnn_amd.config import Config, reconbench_pretrained
    from dgnn_amd.graph import GraphPlan
    from dgnn_amd.learning.surfaceNetStaticEdgeFilters import SurfaceNet

    if args.gemm_mode is not None:
        ops.GEMM_MODE = ops.GEMM_MODE_NAMES[args.gemm_mode]
    if args.widths:
        convs = tuple(int(v) for v in args.widths.split(","))
        torch.manual_seed(0)
        net = SurfaceNet(reconbench_pretrained(device=dev, convs=convs))
        # random-init BatchNorm has unit statistics; give the running buffers some spread so the folded epilogue is exercised
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
        weights = "random init (torch.manual_seed(0)) %s" % (list(convs),)
    else:
        convs = (64, 128, 128, 128)
        net = SurfaceNet(reconbench_pretrained(device=dev, convs=convs))
        net.load_state_dict(load_weights())
        weights = "kf96 checkpoint [64,128,128,128]"
    net_sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net = net.to(dev).eval()
    bf16 = args.dtype == "bf16"
    if bf16:
        net.set_storage_dtype(torch.bfloat16)
    elem = 2 if bf16 else 4

    def sync():
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
        torch.cuda.synchronize()

    def settle(step_fn):
        # Set-up, not warm-up: two untimed steps so that every buffer a step allocates has been touched once.  The first process on a fresh
        # GPU box pays for first touches of VRAM inside its kernels (measured at 10M tets, 20 GB live per step: 44-80 ms instead of 20.8 when
        # the timed steps were the first to hold all layers' outputs at once); the W warm-up steps the contract asks for follow as given.
        for _ in range(2):
            step_fn()
        # ... and the buffers of the per-layer calls an INSTRUMENTED timed step makes (ops.LAYER_HOOK set: the whole-scene call steps aside): left
        # untouched, the first instrumented step of the timed region paid the first touches (10M tets: mean 37 ms over a 13.7 ms median)
        ops.LAYER_HOOK = lambda tok, c_in, c_out, n_dst, plain=True: None
        try:
            for _ in range(2):
                step_fn()
        finally:
            ops.LAYER_HOOK = None
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            step_fn()

    scene_cpu = None
    transport = None
    if world == 1:
        adj, cent, x, ea = make_scene(args.points, 0)
        n_total = n_local = adj.shape[0] // 4
        ei_cpu = torch.from_numpy(adj.T.astype(np.int64))
        scene_cpu = (x, ea, ei_cpu)
        data_gen = Config(x=x.to(dev), edge_attr=ea.to(dev), edge_index=ei_cpu.to(dev))      # the generator's own cell order
        cell_order = None
        if args.cell_order == "loader":
            # the scene as dgnn_amd.processing.data.dataLoader hands it to the model: cells relabelled once at ingest (Morton order of the cell
            # centroids, csrc/reorder.hip -- the reference's loader keeps CGAL's insertion order, processing/data.py:434-438); per-cell results
            # return to file order through the kept permutation (the check below compares in FILE order)
            from dgnn_amd.processing.reorder import reorder_edges, scene_order
            cell_order = scene_order(data_gen.edge_index, n_total, centroids=torch.from_numpy(cent).to(dev), kind="morton")
            ei_o, rows_o = reorder_edges(data_gen.edge_index, cell_order.order, cell_order.rank)
            data = Config(x=ops.gather_rows(data_gen.x, cell_order.order), edge_attr=ops.gather_rows(data_gen.edge_attr, rows_o), edge_index=ei_o)
            del rows_o
        else:
            data = data_gen
        cached = {}

        def step():
            plan = cached.get("p")
            if plan is None:
                plan = GraphPlan(data.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE)
                if args.cached_plan:
                    cached["p"] = plan
            return net.inference_layer(data, plan=plan)
        workload = "synthetic Delaunay tet graph, %d points -> N=%d tets, E=%d, whole-graph inference_layer; cells in %s" % (
            args.points, n_total, 4 * n_total, "the order the package's loader leaves them in (ingest-time Morton order of the cell centroids, "
            "dgnn_amd/processing/reorder.py; `generator_order` = the same scene as generated)" if cell_order is not None else "the generator's order")
    else:
        import torch.distributed as dist
        from dgnn_amd.partition import HaloExchange, PartitionedScene
        gloo = dist.new_group(backend="gloo")     # host-side traffic of the bench itself (flags, the gathered logits of the check)
        transport = "RCCL" if backend == "nccl" else "host-staged %s (validation run, not a benchmark)" % backend    # (refined below once the scene exists)
        host_staged = [False]

        def build_scene(mode):
            total_points = args.points * world if mode == "weak" else args.points
            sc = PartitionedScene.build_synthetic(total_points, 0, rank, world, dev, keep_global=True, halo=args.halo, hops=net.num_layers)
            if host_staged[0]:
                sc.exchange = HaloExchange(sc.lp, dev, pack=ops.gather_rows, group=gloo, via_host=True)
            return sc, total_points
        scene, total_points = build_scene(args.scaling)
        n_total, n_local = scene.n_total, scene.n_own
        rings = args.halo == "recompute"
        if rings:
            transport = "none in the data path"
        elif backend == "nccl":
            transport = ("RCCL, one send / recv group per layer issued by the library on its side stream (dgnn_halo_exchange_start / _wait)"
                         if getattr(scene.exchange, "_native", None) is not None else "RCCL through torch.distributed.batch_isend_irecv")

        def step():
            return scene.inference_layer(net)
        if (backend == "nccl" or os.environ.get("DGNN_BENCH_SAFETY_NET") == "1") and not rings:
            # Safety net: if the device-to-device exchange cannot run on this node (P2P/IPC disabled ...), every rank sees the
            # error in its first step; all ranks then agree to stage the halo rows through host memory over gloo, and the
            # JSON line says so.  Compute is unchanged.
            failed_x = 0
            try:
                step()
                torch.cuda.synchronize()
            except Exception as e:  # noqa: BLE001
                failed_x = 1
                sys.stderr.write("rank %d: RCCL halo exchange failed (%s)\n" % (rank, e))
            flag = torch.tensor([failed_x])
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=gloo)
            if int(flag.item()):
                host_staged[0] = True
                scene.exchange = HaloExchange(scene.lp, dev, pack=ops.gather_rows, group=gloo, via_host=True)
                transport = "host-staged gloo (RCCL point-to-point failed on this node)"
        if rings:
            workload = ("synthetic Delaunay scene, %d points -> N=%d tets, %d-way spatial partition (%s scaling); every part keeps %d rings of halo cells resident and "
                        "recomputes each layer on the rings later layers read (this rank: %d owned cells + rings %s): no collective in the data path, one "
                        "library call per step (dgnn_static_infer_rings_fwd)%s" % (
                            total_points, n_total, world, args.scaling, net.num_layers, n_local, scene.lp.ring_counts,
                            "" if backend == "nccl" else "; validation run under %s (ranks may share a device), not a benchmark" % backend))
        else:
            workload = "synthetic Delaunay scene, %d points -> N=%d tets, %d-way spatial partition (%s scaling) + %s halo exchange overlapped with interior cells" % (
                total_points, n_total, world, args.scaling, transport)

    settle(step)
    # ---- per-kernel breakdown (outside the timed region): replay each layer between events ----
    breakdown = {}
    if world == 1 and not args.no_breakdown:
        plan = GraphPlan(data.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE)

        def timed(fn, reps=10):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps
        breakdown["plan_ms"] = timed(lambda: GraphPlan(data.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE), 5)
        h = net._input_rows(data.x)
        if bf16 and net._storage_input(h).dtype != h.dtype:
            breakdown["cast_ms"] = timed(lambda: ops.cast_to_bf16(h))
            h = ops.cast_to_bf16(h)
        for i in range(net.num_layers):
            if net.fuses_decoder(i):
                breakdown["layer%d_and_decoder_ms" % i] = timed(lambda h=h, i=i: net._eval_layers(h, n_local, data.edge_attr, [plan] * net.num_layers, True, only=i, decode=True))
                break
            fn = lambda h=h, i=i: net._eval_layers(h, n_local, data.edge_attr, [plan] * net.num_layers, True, only=i)
            breakdown["layer%d_ms" % i] = timed(fn)
            h = fn()
        else:
            breakdown["decoder_ms"] = timed(lambda: net._eval_decoder(h))

    # HIP events around EVERY conv layer launch inside the timed region, recorded on the stream the kernels are launched on (torch's current stream),
    # keyed by (c_in, c_out, plain): `plain` = the layer kernel proper, not plain = the last layer's launch that also carries the decoder.  The roofline
    # object describes the kind of launch with the largest share of the step; the other kind of the same shape is nested under `roofline.also`.
    layer_events = {}

    def make_hook(store):
        def hook_(tok, c_in, c_out, n_dst, plain=True):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            if tok is None:
                return ev
            store.setdefault((c_in, c_out, bool(plain)), []).append((tok, ev, n_dst))
            return None
        return hook_
    hook = make_hook(layer_events)
    # N = 1: the events sit inside the timed steps.  N > 1: a shard of the scene is small enough for the per-launch events (and the per-layer calls they
    # need: the product's step there is ONE library call) to show in the step time, so the timed region runs the product's step as it is and the same
    # number of instrumented steps follows it for the roofline object.
    # The events cost the step 1-2 % (eight markers in the queue and the per-layer calls they need -- the product's step is ONE library call): every
    # `--events-every`-th timed step carries them (default 4: 5 of the 20 default steps), the others run the step exactly as a user's call does.
    events_in_timed = world == 1
    inst = {"i": 0, "n": 0}
    every = max(1, args.events_every)

    def step_timed():
        on = inst["i"] % every == 0
        inst["i"] += 1
        if not on:
            return step()
        inst["n"] += 1
        ops.LAYER_HOOK = hook
        try:
            return step()
        finally:
            ops.LAYER_HOOK = None
    last = {} if args.dump_outputs else None
    dt, per_step = timed_steps(step_timed if events_in_timed else step, args.steps, sync, world, dev, keep=last)
    if last is not None:
        dump_output(args.dump_outputs, "logits" if world == 1 else "logits_rank%d" % rank, last.pop("out"), budget=DUMP_BUDGET_BYTES // world)
    if not events_in_timed:
        ops.LAYER_HOOK = hook
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
    ops.LAYER_HOOK = None
    n_inst = inst["n"] if events_in_timed else args.steps      # steps that carried events
    ms_per_step = dt / args.steps * 1e3
    value = n_total * args.steps / dt

    # ---- roofline of the dominant kind of launch: HIP events on the launch stream, inside the timed steps ----
    def roofline_of(layer_events, net, bf16, n_inst, ms_per_step, value, timing_text):
        """the `roofline` object from the per-launch events of `n_inst` instrumented steps of `net` (storage bf16 or fp32) on the n_local cells"""
        elem = 2 if bf16 else 4
        dtype_name = "bf16" if bf16 else "f32"

        def kind_stats(key):
            evs = layer_events[key]
            tot = sum(a.elapsed_time(b) for a, b, _ in evs)
            rows = sum(r for _, _, r in evs)
            # launches of this kind per step (a partitioned layer is two launches, interior + boundary cells: `rows` adds them up so that bytes and
            # time cover the same cells)
            n_l = max(1, round(rows / (n_local * n_inst)))
            ms = tot / (n_l * n_inst)
            c_in, c_out, plain = key
            # SURVEY 8d per-unit figure of what this launch executes: the layer's row, plus the decoder's row (elem * C + 8) when it rides along
            per_tet = layer_bytes(c_in, c_out, elem) + (0 if plain else elem * c_out + 8)
            algo = int(per_tet * rows / (n_l * n_inst))
            return {"total_ms": tot, "launches_per_step": n_l, "ms": ms, "algo": algo, "per_tet": per_tet, "rows_per_launch": rows / (n_l * n_inst), "n_events": len(evs)}

        stats = {k: kind_stats(k) for k in layer_events}
        dom_key = max(stats, key=lambda k: stats[k]["total_ms"])
        traffic_json = None
        try:
            cands = [c_ for c_ in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))
                     if json.load(open(c_)).get("dtype", "f32") == dtype_name]
            traffic_json = (cands[-1], json.load(open(cands[-1])))
        except Exception:  # noqa: BLE001
            pass

        def describe(key):
            st = stats[key]
            c_in, c_out, plain = key
            shape = (c_in, c_out)
            achieved = st["algo"] / (st["ms"] * 1e-3) / 1e9
            fused = ops.fused_layer_supported(c_in, c_out, 20)
            wide_sr = (not bf16) and (not fused) and wide_layer_is_split_rows(net, c_in, c_out)
            if bf16:
                kname = net.dominant_kernel_name(shape)
                if plain and shape in ((128, 128), (64, 128)) and ops.lib().dgnn_wave_specialised_enabled() == 1 and os.environ.get("DGNN_WS_16", "1") != "0" \
                        and ops.BF16_UNSIGNED_ROWS and ops.BF16_MODE == ops.BF16_COMPENSATED:
                    kname = "k_sage_fused_ws<%d,%s,counters,plain,16-bit rows>" % (c_in, "2")     # csrc/fused_ws.hip on the unsigned 16-bit rows
            elif fused:
                kname = {0: "k_sage_fused<%d,%d,0>", 1: "k_sage_fused<%d,%d,1>", 2: "k_sage_fused_mfma<%d,%d>", 3: "k_sage_fused_mfma<%d,%d,dense f16x2>",
                         4: "k_sage_fused_mfma<%d,%d,f16x2>"}[ops.GEMM_MODE] % (32 if c_in <= 32 else (64 if c_in <= 64 else 128), c_out)
                ws = ops.GEMM_MODE == ops.GEMM_F16X2 and shape in ((128, 128), (64, 128)) and ops.lib().dgnn_wave_specialised_enabled() == 1
                if ws:
                    # csrc/fused_ws.hip: 8 producer + 8 consumer wavefronts per workgroup, rows handed over in an LDS ring (DGNN_WS=0: the two-phase kernel)
                    kname = "k_sage_fused_ws<%d,%s,counters,%s>" % (c_in, "2", "plain" if plain else "DEC")
                if not plain:
                    kname = (kname if ws else kname[:-1] + ",DEC>") + " (last conv layer + decoder in one launch)"
            elif wide_sr:
                kname = "k_agg_fwd_sr + k_gemm_sr (aggregate + GEMM on split rows, %d->%d)" % shape
            else:
                kname = "k_agg_fwd + k_linear_fwd (unfused aggregate + GEMM pair, %d->%d)" % shape
            # HBM bytes per launch from the committed rocprofv3 PMC passes (FETCH_SIZE doubled per the gfx950 note + WRITE_SIZE), valid only for
            # the kernel sources they were measured on and for the shape that was profiled
            traffic, pmc, tsrc = None, {}, None
            if traffic_json is not None:
                path, tj = traffic_json
                tsrc = {"file": os.path.relpath(path, ROOT), "commit": tj.get("commit"), "csrc_sha": tj.get("csrc_sha")}
                same_kernel = tj.get("csrc_sha") == csrc_sha()
                same_shape = tuple(tj.get("shape", (128, 128))) == shape and tj.get("dtype", "f32") == dtype_name and (fused or bf16)
                tsrc["matches_this_build"] = bool(same_kernel)
                src_ = tj if plain else (tj.get("with_decoder") or {})
                if same_shape and same_kernel and src_.get("traffic_bytes_per_launch"):
                    traffic = round(src_["traffic_bytes_per_launch"] * st["rows_per_launch"] / tj.get("n_tets", 1010078))
                    pmc = {k: src_[k] for k in ("mfma_busy_frac", "valu_busy_frac", "wait_any_frac", "tcc_hit_rate", "clock_ghz") if k in src_}
                elif same_shape and not same_kernel:
                    sys.stderr.write("bench: %s was measured on other kernel sources (csrc %s, now %s): roofline.traffic left null\n" % (
                        tsrc["file"], tj.get("csrc_sha"), csrc_sha()))
            r = {"bound": "hbm", "kernel": "%s (%d launch%s per step)" % (kname, st["launches_per_step"], "" if st["launches_per_step"] == 1 else "es"),
                 "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                 "traffic": traffic, "traffic_source": tsrc, "algorithmic_bytes_per_launch": st["algo"], "algorithmic_bytes_per_tet": st["per_tet"],
                 "avg_launch_ms": round(st["ms"], 4), "share_of_step": round(st["total_ms"] / n_inst / ms_per_step, 4),
                 "timing": timing_text % st["n_events"], "pmc": pmc or None}
            if not plain:
                # the contract figure counts the layer's output write and the decoder's read of it; the fused launch never moves them (VERDICT r4 weak #11:
                # `frac` is "credit for bytes removed"; `frac_fused` is the fraction of HBM bandwidth the launch actually asks for)
                fused_per_tet = st["per_tet"] - 2 * elem * c_out
                r["fused_bytes_per_tet"] = fused_per_tet
                r["frac_fused"] = round(achieved * fused_per_tet / st["per_tet"] / HBM_PEAK_GBS, 4)
                r["algorithmic_bytes_note"] = ("SURVEY 8d rows this launch executes: last conv layer %d B/tet + decoder %d B/tet (the contract figure, `frac`); the launch itself "
                                               "moves %d B/tet less -- the layer's output never leaves the compute unit -- i.e. `fused_bytes_per_tet`, at `frac_fused` of HBM"
                                               % (layer_bytes(c_in, c_out, elem), elem * c_out + 8, 2 * elem * c_out))
            if not fused and not bf16:
                # a wide layer (aggregate + GEMM pair): 4*C_in*C_out FLOPs per tet against ~4*(C_in+C_out) bytes -- the matrix cores
                # bound it, not HBM.  The yardstick is the rate the arithmetic that actually runs can reach: fp32-class products executed
                # as 6 bf16 (exact 3-way split) or 3 fp16 (2 parts, power-of-two row scales) matrix products each -> dense 16-bit peak / 6
                # or / 3 in fp32-equivalent TFLOP/s; the bit-faithful mode runs on the fp32 matrix pipe itself.
                fl = layer_flops(c_in, c_out) * st["rows_per_launch"]
                tf = fl / (st["ms"] * 1e-3) / 1e12
                x3 = ops.GEMM_MODE != ops.GEMM_F32
                x2h = wide_sr or (ops.GEMM_MODE == ops.GEMM_F16X2 and c_out > 256)   # ops.linear_fwd: the fp16 two-part GEMM takes the layers wider than 256
                nprod = 3 if x2h else 6
                peak = BF16_MATRIX_PEAK_TF / nprod if x3 else FP32_MATRIX_PEAK_TF
                r.update({"bound": "mfma", "achieved": round(tf, 1), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(tf / peak, 4),
                          "algorithmic_flops_per_launch": int(fl), "hbm_frac": round(achieved / HBM_PEAK_GBS, 4),
                          "note": ("fp32-class arithmetic executed as %d %s MFMA products per fp32 product; peak = %.0f TFLOP/s dense 16-bit matrix peak / %d "
                                   "(fp32-equivalent); for scale: %.2f of the %.1f TFLOP/s fp32 matrix pipe"
                                   % (nprod, "fp16 (2 parts per operand, power-of-two row scales)" if x2h else "bf16 (3 parts per operand)",
                                      BF16_MATRIX_PEAK_TF, nprod, tf / FP32_MATRIX_PEAK_TF, FP32_MATRIX_PEAK_TF)) if x3
                          else "bit-faithful fp32 MFMA (v_mfma_f32_32x32x2_f32)"})
                if x2h and not wide_sr:
                    r["kernel"] = r["kernel"].replace("k_linear_fwd", "k_linear_fwd_x2h_big")
            return r
        roof = describe(dom_key)
        twin = (dom_key[0], dom_key[1], not dom_key[2])
        if twin in stats:
            roof["also"] = describe(twin)     # the same shape's other kind of launch (plain layer <-> layer + decoder)
        cs = [28] + [int(v) for v in net.clf.model.convs]
        roof["whole_path_frac"] = round(value * path_bytes(28, cs[1:], elem) / 1e9 / HBM_PEAK_GBS / world, 4)
        return roof

    roof = None
    if layer_events:
        roof = roofline_of(layer_events, net, bf16, n_inst, ms_per_step, value,
                           ("HIP events around each launch inside the timed steps, every %d-th step (%%d launches)" % every) if events_in_timed else
                           "HIP events around each launch in K instrumented steps right behind the timed region (%d launches)")

    # ---- side measurements, outside the timed region (nested objects; never `value`) ----
    extras = {}
    if not args.no_extras:
        extras["gpu_state"] = load_probe(step) if world == 1 else None
    if world == 1 and not args.no_extras and not bf16 and args.widths is None:
        # (1) the bit-faithful build of the same path: fp32 matrix cores, fmaf chains (the headline's products are fp16 two-part)
        old_mode, ops.GEMM_MODE = ops.GEMM_MODE, ops.GEMM_F32
        try:
            settle(step)
            dt_x, ps_x = timed_steps(step, args.steps, sync, world, dev)
            extras["exact_f32"] = {"gemm": "fp32 matrix cores (dense product v_mfma_f32_32x32x2_f32, filter product v_mfma_f32_16x16x4_f32), bit-faithful fmaf chains: --gemm-mode f32", "ms_per_step": round(dt_x / args.steps * 1e3, 4),
                                   "ms_per_step_median": round(float(np.median(ps_x)), 4), "value": round(n_total * args.steps / dt_x, 1), "_logits": (cell_order.to_file(step()) if cell_order is not None else step()).float().cpu()}
            # its own roofline: this leg is matrix-core work in the reference's own arithmetic -- algorithmic FLOPs of the whole path
            # (lin_e on 4 edges, the product-sum, lin_j + lin_i per conv layer; the decoder's two Linears) against the fp32-input MFMA peak
            cs_x = [28] + [int(v) for v in net.clf.model.convs]
            fl_tet = sum(layer_flops(a_, b_) for a_, b_ in zip(cs_x[:-1], cs_x[1:])) + 2 * cs_x[-1] * 64 + 2 * 64 * 2
            tf_x = fl_tet * extras["exact_f32"]["value"] / 1e12
            extras["exact_f32"]["roofline"] = {"bound": "mfma", "achieved": round(tf_x, 1), "peak": FP32_MATRIX_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf_x / FP32_MATRIX_PEAK_TF, 4),
                                               "algorithmic_flops_per_tet": int(fl_tet), "kernel": "k_sage_fused<CIN,COUT,0,1> in --gemm-mode f32 (all four conv launches) + k_decoder_rows",
                                               "hbm_frac": round(extras["exact_f32"]["value"] * path_bytes(28, cs_x[1:], 4) / 1e9 / HBM_PEAK_GBS, 4)}
        finally:
            ops.GEMM_MODE = old_mode
        # (1b) the scene in the generator's own cell order (the headline of rounds 1-3)
        value_gen = value
        if cell_order is not None:
            def step_g():
                return net.inference_layer(data_gen, plan=GraphPlan(data_gen.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE))
            settle(step_g)
            dt_g, ps_g = timed_steps(step_g, args.steps, sync, world, dev)
            value_gen = n_total * args.steps / dt_g
            extras["generator_order"] = {"what": "same scene, cells as scipy.spatial.Delaunay numbered them (median |src - dst| = 6 rows; the `value` of rounds 1-3)",
                                         "ms_per_step": round(dt_g / args.steps * 1e3, 4), "ms_per_step_median": round(float(np.median(ps_g)), 4),
                                         "value": round(value_gen, 1)}
        # (2) the same graph with its cells numbered at random -- the gather locality of a CGAL-ordered real scene
        if n_total <= 3_000_000:
            adj_r, x_r, ea_r = relabelled_scene(adj, x, ea)
            data_r = Config(x=x_r.to(dev), edge_attr=ea_r.to(dev), edge_index=torch.from_numpy(adj_r.T.astype(np.int64)).to(dev))

            def step_r():
                return net.inference_layer(data_r, plan=GraphPlan(data_r.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE))
            settle(step_r)
            dt_r, ps_r = timed_steps(step_r, args.steps, sync, world, dev)
            extras["random_cell_order"] = {"what": "same graph, cells renumbered by a seeded random permutation (no gather locality; the generator's own order has median |src - dst| = 6 rows)",
                                           "ms_per_step": round(dt_r / args.steps * 1e3, 4), "ms_per_step_median": round(float(np.median(ps_r)), 4),
                                           "value": round(n_total * args.steps / dt_r, 1)}
            # (3) that scene through the INGEST-TIME cell order of dgnn_amd.processing (what dataLoader.run does to a real scene, reference seam
            # processing/data.py:434-438): Morton order of the cell centroids (a scene with <scene>_3dt.npz), breadth-first order of the adjacency (none)
            from dgnn_amd.processing.reorder import reorder_edges, scene_order
            perm_r = np.random.default_rng(7).permutation(n_total)      # relabelled_scene's permutation: new id of old cell
            inv_r = np.empty(n_total, np.int64)
            inv_r[perm_r] = np.arange(n_total)
            cent_r = torch.from_numpy(np.ascontiguousarray(cent[inv_r])).to(dev)
            extras["real_order"] = {"what": "the random_cell_order scene after the loader's ingest-time relabelling (dgnn_amd/processing/reorder.py); logits go back to file "
                                            "order through the kept permutation", "generator_order_value": round(value_gen, 1)}
            for kind in ("morton", "bfs"):
                def ingest():
                    co_ = scene_order(data_r.edge_index, n_total, centroids=cent_r if kind == "morton" else None, kind=kind)
                    ei_, rows_ = reorder_edges(data_r.edge_index, co_.order, co_.rank)
                    return co_, Config(x=ops.gather_rows(data_r.x, co_.order), edge_attr=ops.gather_rows(data_r.edge_attr, rows_), edge_index=ei_)
                ingest()
                torch.cuda.synchronize()
                t_i = time.perf_counter()
                co_k, data_k = ingest()
                torch.cuda.synchronize()
                t_i = time.perf_counter() - t_i

                def step_k():
                    return net.inference_layer(data_k, plan=GraphPlan(data_k.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE))
                settle(step_k)
                dt_k, ps_k = timed_steps(step_k, args.steps, sync, world, dev)
                back = co_k.to_file(step_k())
                same = float((back - step_r()).abs().max())            # same graph, sums in another order
                d_k = (data_k.edge_index[0] - data_k.edge_index[1]).abs().float()
                extras["real_order"][kind] = {"ms_per_step": round(dt_k / args.steps * 1e3, 4), "ms_per_step_median": round(float(np.median(ps_k)), 4),
                                              "value": round(n_total * args.steps / dt_k, 1), "vs_generator_order": round(n_total * args.steps / dt_k / value_gen, 4),
                                              "ingest_reorder_ms": round(t_i * 1e3, 2), "median_src_dst_rows": int(d_k.median().item()),
                                              "max_abs_dlogit_vs_unordered": same}
                del data_k, co_k
            del data_r, x_r, ea_r, adj_r, cent_r
        # (4) reconbench-size scenes (BASELINE config 2: run.py:170-191 classifies one ~66k-cell scene after the other): 25 scenes back to back, each
        # ONE library call (plan + layers + decoder, dgnn_static_infer_fwd) on a scene whose plan has never been built, and the same 25 as one
        # block-diagonal batch
        from dgnn_amd.graph import clear_plan_cache
        small = []
        for sd_ in range(5):
            adj_s, _, x_s, ea_s = make_scene(args.small_points, 100 + sd_)
            small.append(Config(x=x_s.to(dev), edge_attr=ea_s.to(dev), edge_index=torch.from_numpy(adj_s.astype(np.int64)).to(dev).t()))
        scenes = [small[i % 5] for i in range(25)]
        n_small = sum(d_.x.size(0) for d_ in scenes)

        def small_pass():
            for d_ in scenes:
                clear_plan_cache(d_.edge_index)
                net.inference_layer(d_)

        def small_timed(fn, reps=8):
            fn()
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0_ = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0_)
            return float(np.median(ts))
        t_one = small_timed(small_pass)
        ops.INFER_ONE_CALL = False
        try:
            t_layers = small_timed(small_pass)
        finally:
            ops.INFER_ONE_CALL = True
        off, xs, eas, eis = 0, [], [], []
        for d_ in scenes:
            xs.append(d_.x); eas.append(d_.edge_attr); eis.append(d_.edge_index.t().contiguous() + off)
            off += d_.x.size(0)
        batch = Config(x=torch.cat(xs), edge_attr=torch.cat(eas), edge_index=torch.cat(eis).t())

        def batch_pass():
            clear_plan_cache(batch.edge_index)
            return net.inference_layer(batch)
        t_batch = small_timed(batch_pass)
        lg_b = batch_pass()
        lg_0 = net.inference_layer(scenes[0])
        extras["small_scenes"] = {"what": "25 scenes of %d tets (%d points each), plan built inside every call" % (scenes[0].x.size(0), args.small_points),
                                  "one_call_ms_per_scene": round(t_one / 25 * 1e3, 4), "one_call_value": round(n_small / t_one, 1),
                                  "per_layer_calls_ms_per_scene": round(t_layers / 25 * 1e3, 4), "per_layer_calls_value": round(n_small / t_layers, 1),
                                  "block_diagonal_batch_ms": round(t_batch * 1e3, 4), "block_diagonal_batch_value": round(n_small / t_batch, 1),
                                  "batch_equals_scene_bitwise": bool(torch.equal(lg_b[:lg_0.size(0)], lg_0))}
        del small, scenes, batch, xs, eas, eis
        # (5) the metric's other GPU counts, one rank at a time on THIS GPU: the step of a rank's part of a W-way cut of this very scene (ring parts,
        # dgnn_amd/partition.py: the ranks do not talk during a step -- no collective in the data path -- so a rank's step time here is its step time
        # there; the W-GPU job additionally pays the timing harness's barrier).  First and last rank of every cut; logits checked against the whole
        # scene's.  `bench.py --gpus W` runs exactly these parts, one per GPU.
        if n_total <= 3_000_000 and cell_order is not None:
            from dgnn_amd.partition import PartitionedScene, build_ring_part, rcb_partition
            ei_np = data.edge_index.cpu().numpy()
            cent_o = cent[cell_order.order.cpu().numpy()]
            whole = step()
            parts_out = {}
            for W in (2, 4, 8):
                part = rcb_partition(cent_o, W)
                ms_w, same_w, own_w, ring_w = [], True, [], []
                for r_ in (0, W - 1):
                    lp = build_ring_part(ei_np, part, r_, W, net.num_layers)
                    rows_ = torch.from_numpy(np.concatenate([lp.own_gid, lp.halo_gid])).to(dev)
                    sc_ = PartitionedScene(lp, data.x[rows_], data.edge_attr[torch.from_numpy(lp.edge_gid).to(dev)], dev)
                    fn_ = lambda sc_=sc_: sc_.inference_layer(net)
                    settle(fn_)
                    k_p = max(args.steps, 100)        # (a shard's step is 0.2-0.8 ms: enough of them to be past the clock ramp that follows the host-side part building)
                    for _ in range(20):
                        fn_()
                    dt_p, _ = timed_steps(fn_, k_p, sync, world, dev)
                    ms_w.append(round(dt_p / k_p * 1e3, 4))
                    same_w = same_w and bool(torch.equal(fn_(), whole[torch.from_numpy(lp.own_gid).to(dev)]))
                    own_w.append(lp.n_own)
                    ring_w.append(lp.ring_counts)
                    del sc_, rows_, lp
                parts_out[str(W)] = {"ms_per_step_rank_first_last": ms_w, "owned_cells": own_w, "rings": ring_w, "bit_identical_to_whole_scene": same_w,
                                     "value_if_every_rank_takes_the_slower": round(n_total / max(ms_w) * 1e3, 1),
                                     "vs_this_gpu": round(n_total / max(ms_w) * 1e3 / value, 3)}
            extras["strong_scaling_parts"] = {"what": "ring parts of the W-way cut of this scene, each timed alone on this GPU (the ranks are independent during a step: no "
                                                      "collective in the data path); `bench.py --gpus W` runs them one per GPU", "steps_per_part": max(args.steps, 100), "parts": parts_out}
            del ei_np, cent_o, whole
        # (6) the other configurations quoted in README / DESIGN under the DRIVER's clock, on the scene of the headline, 10 steps
        # each: bf16 STORAGE (BASELINE config 3's storage type) with its own roofline object, and the widths the reference's real configs use
        # (configs/eth.yaml:56, aerial.yaml:57: [64,128,256,512]; configs/modelnet.yaml:56, shapenet.yaml: [128,256,512,1024]; random init as --widths)
        k_n = min(args.steps, 10)

        def nested_leg(net_n, bf16_n):
            def step_n():
                return net_n.inference_layer(data, plan=GraphPlan(data.edge_index, n_local, n_local, hint=ops.PLAN_HINT_REFERENCE))
            settle(step_n)
            dt_n, ps_n = timed_steps(step_n, k_n, sync, world, dev)
            leg = {"ms_per_step": round(dt_n / k_n * 1e3, 4), "ms_per_step_median": round(float(np.median(ps_n)), 4), "value": round(n_total * k_n / dt_n, 1),
                   "steps": k_n}
            ev_n = {}
            ops.LAYER_HOOK = make_hook(ev_n)
            try:
                for _ in range(5):
                    step_n()
                torch.cuda.synchronize()
            finally:
                ops.LAYER_HOOK = None
            if ev_n:
                leg["roofline"] = roofline_of(ev_n, net_n, bf16_n, 5, dt_n / k_n * 1e3, n_total * k_n / dt_n,
                                              "HIP events around each launch in 5 instrumented steps right behind this leg's timed steps (%d launches)")
            return leg, step_n
        net_b = SurfaceNet(reconbench_pretrained(device=dev, convs=convs))
        net_b.load_state_dict(net_sd)
        net_b = net_b.to(dev).eval()
        net_b.set_storage_dtype(torch.bfloat16)
        leg_b, step_b = nested_leg(net_b, True)
        leg_b["what"] = "the same scene and weights in bf16 STORAGE (`python bench.py --dtype bf16`): 16-bit rows between the layers, fp32 accumulate, decoder in the last launch"
        leg_b["algorithmic_bytes_per_tet"] = path_bytes(28, convs, 2)
        leg_b["_logits"] = (cell_order.to_file(step_b()) if cell_order is not None else step_b()).float().cpu()
        extras["bf16_storage"] = leg_b
        del net_b, step_b
        wide = {}
        for convs_w in ((64, 128, 256, 512), (128, 256, 512, 1024)):
            torch.manual_seed(0)
            net_w = SurfaceNet(reconbench_pretrained(device=dev, convs=convs_w))
            for m in net_w.modules():
                if isinstance(m, torch.nn.BatchNorm1d):
                    m.running_mean.normal_(0, 0.1)
                    m.running_var.uniform_(0.5, 1.5)
            sd_w = {k: v.detach().clone() for k, v in net_w.state_dict().items()}
            net_w = net_w.to(dev).eval()
            leg_w, step_w = nested_leg(net_w, False)
            leg_w["weights"] = "random init (torch.manual_seed(0)) %s" % (list(convs_w),)
            leg_w["algorithmic_bytes_per_tet"] = path_bytes(28, convs_w, 4)
            leg_w["_net"] = (net_w, sd_w, convs_w)
            wide[",".join(str(v) for v in convs_w)] = leg_w
            del step_w
        extras["wide_widths"] = wide
    if scene10 is not None:
        # (7) the 10 026 136-tet scene (BASELINE config 4's size on ONE GPU; `python bench.py --points 1485000` as its own line): same weights and
        # arithmetic, features drawn on the device, cells in the loader's Morton order, plan built inside the step.  The child process has been
        # triangulating since this run started.
        proc10, dir10 = scene10
        budget = 150.0 if args.scene_10m == "auto" else 1e9
        while proc10.poll() is None and time.perf_counter() - t_bench0 < budget - 45.0:
            time.sleep(0.5)
        if proc10.poll() == 0 and os.path.exists(os.path.join(dir10, "done")):
            try:
                from dgnn_amd.processing.reorder import reorder_edges, scene_order
                from dgnn_amd.synthetic import hashed_normal
                adj10 = np.load(os.path.join(dir10, "adj.npy"))
                cent10 = np.load(os.path.join(dir10, "cent.npy"))
                n10 = adj10.shape[0] // 4
                ei10 = torch.from_numpy(adj10).to(dev).to(torch.int64).t()
                x10 = hashed_normal(np.arange(n10), 29, seed=1, device=dev)
                ea10 = hashed_normal(np.arange(4 * n10), 20, seed=2, device=dev)
                co10 = scene_order(ei10, n10, centroids=torch.from_numpy(cent10).to(dev), kind="morton")
                ei10o, rows10 = reorder_edges(ei10, co10.order, co10.rank)
                data10 = Config(x=ops.gather_rows(x10, co10.order), edge_attr=ops.gather_rows(ea10, rows10), edge_index=ei10o)
                del x10, ea10, ei10, rows10, adj10, cent10

                def step10():
                    return net.inference_layer(data10, plan=GraphPlan(data10.edge_index, n10, n10, hint=ops.PLAN_HINT_REFERENCE))
                settle(step10)
                k10 = min(args.steps, 10)
                dt10, ps10 = timed_steps(step10, k10, sync, world, dev)
                lg10 = step10()
                extras["scene_10m"] = {"what": "synthetic Delaunay scene, 1485000 points -> %d tets on ONE GPU, loader's Morton cell order, plan in the step, kf96 weights" % n10,
                                       "n_tets": n10, "steps": k10, "ms_per_step": round(dt10 / k10 * 1e3, 4), "ms_per_step_median": round(float(np.median(ps10)), 4),
                                       "value": round(n10 * k10 / dt10, 1), "logits_finite": bool(torch.isfinite(lg10).all().item()),
                                       "whole_path_frac": round(n10 * k10 / dt10 * path_bytes(28, convs, elem) / 1e9 / HBM_PEAK_GBS, 4),
                                       "parity": "tests/test_gpu_multi.py: this scene's 8 parts equal the whole graph bit for bit; the arithmetic is the headline's (checked against the oracle)"}
                del data10, lg10, co10, ei10o
                torch.cuda.empty_cache()
            except Exception as e:  # noqa: BLE001 -- a side leg must not cost the line
                extras["scene_10m"] = {"skipped": "failed: %r" % (e,)}
        else:
            extras["scene_10m"] = {"skipped": "the scene's triangulation (about a minute of one host core) was not ready %.0f s into the run: "
                                              "`python bench.py --points 1485000` or `--scene-10m on` measures it" % (time.perf_counter() - t_bench0)}
        drop_scene_builder(scene10)
        scene10 = None
    other = None
    if world > 1 and not args.no_extras:
        # the other scaling mode, same steps / warm-up, so that a SCALE record can be read either way (metric: "1M-tet graph at 1/2/4/8" = strong)
        o_mode = "strong" if args.scaling == "weak" else "weak"
        scene_o, points_o = build_scene(o_mode)

        def step_o():
            return scene_o.inference_layer(net)
        settle(step_o)
        dt_o, ps_o = timed_steps(step_o, args.steps, sync, world, dev)
        other = {"scaling": o_mode, "value": round(scene_o.n_total * args.steps / dt_o, 1), "ms_per_step": round(dt_o / args.steps * 1e3, 4),
                 "ms_per_step_median": round(float(np.median(ps_o)), 4), "n_tets": scene_o.n_total, "tets_per_gpu": scene_o.n_own, "points": points_o}
    # north_star's form of the partitioned forward -- "RCCL halo exchange of boundary-tet features over xGMI each message-passing round" (what replaces
    # run.py:221-223's per-batch k-hop recomputation) -- timed beside the ring-parts `value` in EVERY multi-GPU line: one ring of
    # halo rows, rows exchanged before conv layers 1..3 by the library's RCCL send / recv group on its side stream (dgnn_halo_exchange_start / _wait),
    # interior cells computed meanwhile.  Same scene as `value`; logits checked bit for bit against a single-rank run like the headline's.
    legs_x = {}
    if world > 1 and not args.no_extras and args.halo == "recompute":
        def exchange_leg(points_x, label):
            sc_x = PartitionedScene.build_synthetic(points_x, 0, rank, world, dev, keep_global=True, halo="exchange", hops=net.num_layers)
            tr_x = "host-staged %s (validation run, not a benchmark)" % backend
            if backend == "nccl" or os.environ.get("DGNN_BENCH_SAFETY_NET") == "1":
                failed_x = 0
                try:
                    sc_x.inference_layer(net)
                    torch.cuda.synchronize()
                except Exception as e:  # noqa: BLE001 -- same safety net as the --halo exchange headline
                    failed_x = 1
                    sys.stderr.write("rank %d: RCCL halo exchange failed (%s)\n" % (rank, e))
                flag = torch.tensor([failed_x])
                dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=gloo)
                if int(flag.item()):
                    sc_x.exchange = HaloExchange(sc_x.lp, dev, pack=ops.gather_rows, group=gloo, via_host=True)
                    tr_x = "host-staged gloo (RCCL point-to-point failed on this node)"
                else:
                    tr_x = ("RCCL, one send / recv group per layer issued by the library on its side stream (dgnn_halo_exchange_start / _wait)"
                            if getattr(sc_x.exchange, "_native", None) is not None else "RCCL through torch.distributed.batch_isend_irecv")

            def step_x():
                return sc_x.inference_layer(net)
            settle(step_x)
            dt_x, ps_x = timed_steps(step_x, args.steps, sync, world, dev)
            nat = getattr(sc_x.exchange, "_native", None)
            rccl_world = None
            if nat is not None:
                from dgnn_amd._lib import lib
                rccl_world = int(lib().dgnn_comm_count(nat[1]))
            leg = {"what": "%s: one ring of halo rows, exchanged before conv layers 1..%d, interior cells computed meanwhile" % (label, net.num_layers - 1),
                   "ms_per_step": round(dt_x / args.steps * 1e3, 4), "ms_per_step_median": round(float(np.median(ps_x)), 4),
                   "value": round(sc_x.n_total * args.steps / dt_x, 1), "n_tets": sc_x.n_total, "tets_per_gpu": sc_x.n_own,
                   "halo_rows_this_rank": int(sc_x.n_halo), "transport": tr_x, "rccl_world": rccl_world}
            return leg, sc_x
        leg_x, scene_x = exchange_leg(args.points if args.scaling == "strong" else args.points * world, "the scene of `value` in the exchange form")
        legs_x["halo_exchange"] = (leg_x, scene_x)
        if world == 8 and backend == "nccl" and os.environ.get("DGNN_BENCH_CONFIG4", "1") != "0":
            # BASELINE config 4 at its size: the 1 485 000-point scene (10 026 136 tets), 8-way partition + RCCL halo exchange
            leg_4, scene_4 = exchange_leg(1485000, "BASELINE config 4: synthetic 10M-tet scene, 8-way graph partition")
            legs_x["config4_10m"] = (leg_4, scene_4)

    # ---- CPU baseline (the oracle on the host cores) + self-check of the GPU logits against it ----
    cpu, check, failed = None, None, False
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        # 16 threads is where this op chain peaks on the GPU host (tools/cpu_sweep.py: 1 -> 9.7e4, 16 -> 1.6e5,
        # 64 -> 1.1e5, 128 -> 6.7e4 tets/s on a 256-core box): more threads only add contention
        cores = min(os.cpu_count() or 1, 16)
        x_c, ea_c, ei_c = scene_cpu
        big = n_total > 3_000_000           # 10M-tet runs: the oracle would need >100 GB of [E,C] temporaries; use a sample
        if big:
            adj_s, _, x_c, ea_c = make_scene(150000, 0)
            ei_c = torch.from_numpy(adj_s.T.astype(np.int64))
        t_full, ref = cpu_oracle(net_sd, convs, x_c, ea_c, ei_c, cores, runs=3 if x_c.shape[0] < 1_500_000 else 1)
        n_full = x_c.shape[0]
        adj_1, _, x_1, ea_1 = make_scene(args.cpu_points, 0)
        t_one, _ = cpu_oracle(net_sd, convs, x_1, ea_1, torch.from_numpy(adj_1.T.astype(np.int64)), 1, runs=1)
        cpu = {"value": round(n_full / t_full, 1), "unit": "tets/s", "cores": cores, "kind": "port",
               "sample": "oracle (PyTorch-CPU restatement of inference_layer) on %s (%d tets), %d threads, 1 warm-up + median of 3"
                         % ("the benchmarked graph itself" if not big else "the 150000-point metric graph", n_full, cores),
               "single_thread_value": round(x_1.shape[0] / t_one, 1),
               "single_thread_sample": "same generator at %d points -> %d tets, 1 thread, 1 warm-up + 1 run" % (args.cpu_points, x_1.shape[0])}
        all_cores = os.cpu_count() or 1
        if all_cores > cores and not args.no_extras:
            t_all, _ = cpu_oracle(net_sd, convs, x_c, ea_c, ei_c, all_cores, runs=-1)
            cpu["all_cores_value"] = round(n_full / t_all, 1)
            cpu["all_cores"] = all_cores
            cpu["all_cores_sample"] = "same graph, torch.set_num_threads(%d) = every host core, one run (the 16-thread leg before it has warmed the allocator; more threads than %d only add contention here)" % (all_cores, cores)
        # the check: GPU logits of the same graph against the oracle's
        if big:
            got = net.inference_layer(Config(x=x_c.to(dev), edge_attr=ea_c.to(dev), edge_index=ei_c.to(dev))).float().cpu()
        else:
            got = step()
            got = (cell_order.to_file(got) if cell_order is not None else got).float().cpu()      # logits back in file order
        check = {"reference": "CPU oracle, same graph and weights (%d tets)" % n_full}
        check.update(logits_check(got, ref, bf16, ops.BF16_MODE == ops.BF16_COMPENSATED))
        failed = not check["ok"]
        if "exact_f32" in extras and not big:
            c_x = logits_check(extras["exact_f32"]["_logits"], ref, False)
            extras["exact_f32"]["check"] = {k: c_x[k] for k in ("max_abs_err", "rms_err", "argmax_flips", "ok")}
            failed = failed or not c_x["ok"]
        if "bf16_storage" in extras and not big:
            c_b = logits_check(extras["bf16_storage"]["_logits"], ref, True, ops.BF16_MODE == ops.BF16_COMPENSATED)
            extras["bf16_storage"]["check"] = c_b
            failed = failed or not c_b["ok"]
        for key_w, leg_w in (extras.get("wide_widths") or {}).items():
            # these widths against the CPU oracle on the single-thread leg's sample scene (the oracle's [E, C] temporaries at 512-1024 channels: 1.6 GB there)
            net_w, sd_w, convs_w = leg_w["_net"]
            _, ref_w = cpu_oracle(sd_w, convs_w, x_1, ea_1, torch.from_numpy(adj_1.T.astype(np.int64)), cores, runs=0)
            got_w = net_w.inference_layer(Config(x=x_1.to(dev), edge_attr=ea_1.to(dev), edge_index=torch.from_numpy(adj_1.T.astype(np.int64)).to(dev))).float().cpu()
            c_w = logits_check(got_w, ref_w, False)
            leg_w["check"] = dict(reference="CPU oracle, same weights, the %d-tet sample scene" % x_1.shape[0], **{k: c_w[k] for k in ("max_abs_err", "rms_err", "tolerance", "argmax_flips_above_margin", "ok")})
            failed = failed or not c_w["ok"]
    if "exact_f32" in extras:
        extras["exact_f32"].pop("_logits", None)
    if "bf16_storage" in extras:
        extras["bf16_storage"].pop("_logits", None)
    for leg_w in (extras.get("wide_widths") or {}).values():
        leg_w.pop("_net", None)
    if world > 1:
        # N > 1: every rank's logits of its own cells go to rank 0, which runs the SAME scene on its own GPU as one whole graph (single-rank path,
        # same kernels) -- the partitioned result must equal it bit for bit -- and, when the scene is small enough for the host, the CPU oracle.
        import torch.distributed as dist
        from dgnn_amd.synthetic import hashed_normal

        def gathered_check(sc, label):
            mine = (torch.from_numpy(sc.lp.own_gid), sc.inference_layer(net).float().cpu())
            parts = [None] * world if rank == 0 else None
            dist.gather_object(mine, parts, dst=0, group=gloo)
            if rank != 0:
                return None
            n = sc.n_total
            got = torch.full((n, 2), float("nan"))
            for gid, lg in parts:
                got[gid] = lg
            ei = torch.empty((2, 4 * n), dtype=torch.int64)
            ei[0] = torch.arange(n).repeat_interleave(4)
            ei[1] = torch.from_numpy(sc.global_dst.astype(np.int64))
            xw, eaw = hashed_normal(np.arange(n), 29, seed=1, device=dev), hashed_normal(np.arange(4 * n), 20, seed=2, device=dev)
            whole = net.inference_layer(Config(x=xw, edge_attr=eaw, edge_index=ei.to(dev))).float().cpu()
            res = {"scene": label, "n_tets": n, "reference": "rank 0: the same scene as ONE whole graph on its GPU (single-rank inference_layer)",
                   "bit_identical_to_single_rank": bool(torch.equal(got, whole)), "max_abs_diff_vs_single_rank": float((got - whole).abs().max()),
                   "cells_covered": int(torch.isfinite(got).all(1).sum())}
            res["ok"] = res["bit_identical_to_single_rank"] and res["cells_covered"] == n
            if n <= 1_500_000 and not args.no_cpu_baseline:
                _, ref = cpu_oracle(net_sd, convs, xw.cpu(), eaw.cpu(), ei, min(os.cpu_count() or 1, 16), runs=0)
                c_o = logits_check(got, ref, bf16, ops.BF16_MODE == ops.BF16_COMPENSATED)
                res["vs_cpu_oracle"] = c_o
                res["ok"] = res["ok"] and c_o["ok"]
            return res
        check = gathered_check(scene, "%s scaling, %d tets" % (args.scaling, scene.n_total))
        if other is not None:
            c2 = gathered_check(scene_o, "%s scaling, %d tets" % (other["scaling"], scene_o.n_total))
            if rank == 0:
                other["check"] = c2
        for key_x, (leg_x, scene_x) in legs_x.items():
            big_x = scene_x.n_total > 3_000_000
            c_x = gathered_check(scene_x, "%s, %d tets" % (key_x, scene_x.n_total)) if not big_x else None
            if rank == 0:
                # (the 10M-tet scene's whole-graph reference does not fit the check's budget on one rank: covered by
                # tests/test_gpu_multi.py::test_config4_10m_tets_eight_parts_equal_the_whole_graph)
                leg_x["check"] = c_x if c_x is not None else {"skipped": "10M-tet whole-graph reference: see tests/test_gpu_multi.py (8 parts bit-identical to the whole graph)"}
        if rank == 0:
            failed = not check["ok"] or (other is not None and not other["check"]["ok"]) or any(
                l_[0].get("check", {}).get("ok") is False for l_ in legs_x.values())

    if rank == 0:
        gemm = {0: "fp32 MFMA", 1: "split-bf16 MFMA for the dense part (3 exact bf16 parts per fp32 operand, 6 products, fp32 accumulate)",
                2: "split-bf16 MFMA for the dense part and the filter MLP (3 exact bf16 parts per fp32 operand, 6 products, fp32 accumulate)",
                3: "dense part: fp32 operands scaled by powers of two and split into 2 fp16 parts (22 bits), 3 products on fp16 MFMA, fp32 accumulate; filter MLP split-bf16 x 3",
                4: "dense part and filter MLP: fp32 operands scaled by powers of two and split into 2 fp16 parts (22 significand bits), 3 products on fp16 MFMA, "
                   "fp32 accumulate (the 3xTF32 scheme)"}[ops.GEMM_MODE]
        if bf16:
            gemm = ("bf16 storage of activations; compensated mode: the fp32 mean / attributes / parameters enter the bf16 MFMAs as (hi, lo) pairs, "
                    "fp32 accumulate; first layer reads the fp32 features in place" if ops.BF16_MODE == ops.BF16_COMPENSATED else
                    "bf16 storage of activations, single-product bf16 MFMA (every operand rounded to bf16 once), fp32 accumulate")
        out = {
            "metric": "tetrahedra/sec (in/out classified), 1M-tet graph at 1/2/4/8 MI355X",
            "value": round(value, 1), "unit": "tets/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4), "ms_per_step_median": round(float(np.median(per_step)), 4),
            "higher_is_better": True, "scaling": args.scaling if world > 1 else "weak", "vs_baseline": None,
            # what the path computes in: fp32 storage + fp32 accumulation, the products as named (VERDICT r3 hygiene: a bare "f32" hid the 22-bit operands)
            "dtype": ("bf16 storage (16-bit rows in HBM, fp32 accumulate, parameters fp32)" if bf16 else
                      {0: "f32", 1: "f32 (bf16x3-split products, 24-bit operands)", 2: "f32 (bf16x3-split products, 24-bit operands)",
                       3: "f32 (fp16x2-split products, 22-bit operands; `exact_f32` = bit-faithful fp32 products)",
                       4: "f32 (fp16x2-split products, 22-bit operands; `exact_f32` = bit-faithful fp32 products)"}[ops.GEMM_MODE]), "data": "synthetic",
            "config": {"workload": workload, "tets_per_gpu": n_local, "weights": weights,
                       "plan_in_step": not args.cached_plan, "gemm": gemm, "algorithmic_bytes_per_tet": path_bytes(28, convs, elem),
                       "decoder": "fused into the last conv layer's launch" if net.fuses_decoder(net.num_layers - 1) else "own launch",
                       "timing": "value = wall clock over the K steps between barrier + synchronize, max over ranks; ms_per_step_median = median of the per-step "
                                 "times from events recorded on the launch stream between the steps (rank 0)",
                       # replays of one layer at a time, outside the timed region: they do not add up to ms_per_step (a layer replayed alone runs 2-5 % slower
                       # than inside the step); the roofline uses events inside the timed steps instead
                       "replay_breakdown_ms": {k: round(v, 4) for k, v in breakdown.items()}},
            "roofline": roof, "cpu_baseline": cpu, "check": check,
        }
        out.update({k: v for k, v in extras.items() if v is not None})
        if other is not None:
            out["other_scaling"] = other
        for key_x, (leg_x, _) in legs_x.items():
            out[key_x] = leg_x
        if world == 1 and not args.no_train and args.widths is None and args.points == 150000:
            # fp32 line: the Static model's step; bf16 line: BASELINE config 3's shape of work (Updated variant, bf16 storage)
            out["training_step"] = training_leg(["--updated", "--dtype", "bf16"] if bf16 else [])
            if not bf16 and not args.no_extras:
                out["training_step_updated_bf16"] = training_leg(["--updated", "--dtype", "bf16"])   # BASELINE config 3's model and storage type
                # the widths and batch size the reference trains ModelNet10 with (configs/modelnet.yaml:44,56: [128,256,512,1024], batch 1024)
                out["training_step_modelnet_widths"] = training_leg(["--widths", "128,256,512,1024", "--batch", "1024", "--steps", "100", "--warmup", "100"])
                # BASELINE config 3 at its own workload: the Updated variant, bf16 storage, ModelNet10's widths and batch size
                out["training_step_updated_bf16_modelnet_widths"] = training_leg(["--updated", "--dtype", "bf16", "--widths", "128,256,512,1024", "--batch", "1024",
                                                                                  "--steps", "100", "--warmup", "100"])
            if not bf16 and not args.no_extras:
                # BASELINE config 3 as a functional check: Updated model, ModelNet10 widths / batch, 300 Adam steps in fp32 storage and in bf16 storage from the
                # same weights on the same blocks (tools/config3_convergence.py; tests/test_gpu_config3.py asserts the same band)
                out["config3_convergence"] = convergence_leg()
        line = json.dumps(headline_of(out, write_full(out)))
        if len(line) > 4096:      # never the driver's problem: drop the optional legs, largest first, until the line fits
            h_ = json.loads(line)
            for k_ in ("strong_scaling_parts", "small_scenes", "gpu_state", "real_order", "wide_widths", "bf16_storage", "exact_f32"):
                if len(json.dumps(h_)) <= 4096:
                    break
                h_.pop(k_, None)
            line = json.dumps(h_)
        print(line)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    if failed:
        sys.stderr.write("bench: GPU logits differ from the reference beyond the stated tolerance: %s\n" % json.dumps(check))
        sys.exit(3)


if __name__ == "__main__":
    main()
