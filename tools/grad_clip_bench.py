#!/usr/bin/env python3
"""Cost of device-side gradient-norm clipping in the ViT3D-base train step (TrainStep(max_grad_norm=...)), one MI355X:

    default         TrainStep(model)                          AdamW where the batch rule puts it (fuse_update 3 up to 4096 token rows)
    fuse_update=0   TrainStep(model, fuse_update=0)           one AdamW launch behind the backward pass - what clipping has to use
    clip            TrainStep(model, max_grad_norm=1.0)       that, plus nv_grad_sumsq + nv_grad_clip_finish and nv_adamw_step_clipped

at batch 4 and batch 32, bf16 and fp16 operands (fp16: with the dynamic loss scale, whose overflow check the clipping pass replaces).
Each variant is timed with device events around `--steps` steps after `--warmup`, `--rounds` times, the variants taking turns inside
every round (other work shares the host: a difference counts only beside the spread between rounds).  The reduction itself is timed
the same way, back to back over the 88.58 M-element gradient arena, beside nv_loss_scale_check, which reads the same bytes.

    python tools/grad_clip_bench.py                         # everything; one JSON line per (batch, operands) and one for the kernels
    python tools/grad_clip_bench.py --batches 4 --operands bf16
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/grad_clip_bench.py --trace      # a few clipped steps, nothing timed
    python tools/grad_clip_bench.py --stats OUT/.../kernel_stats.csv                          # the reduction kernel's own duration from that run
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3                                   # achievable HBM bandwidth of the MI355X (TB/s)
VARIANTS = (("default", {}), ("fuse_update=0", {"fuse_update": 0}), ("clip", {"max_grad_norm": 1.0}))
KERNELS = {"grad_sumsq": "grad_sumsq_kernel", "grad_sumsq_partials": "grad_sumsq_finish_kernel", "grad_clip_finish": "grad_clip_finish_kernel",
           "grad_check": "grad_check_kernel", "adamw": "adamw_kernel"}


def byte_floor_us(count, bytes_per=4):
    return count * bytes_per / (HBM_TBS * 1e12) * 1e6


def stats(path, count):
    rows = list(csv.DictReader(open(path)))
    out = {"arena_elements": count, "byte_floor_us": round(byte_floor_us(count), 1)}
    for tag, name in KERNELS.items():
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out[tag] = {"calls": calls, "mean_us": round(sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e3, 2)}
    if "grad_sumsq" in out:
        out["grad_sumsq_over_floor"] = round(out["grad_sumsq"]["mean_us"] / byte_floor_us(count), 3)
    print(json.dumps(out), flush=True)


def make_model(operands):
    import torch
    from neurovit_amd import config as nvcfg
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    size = nvcfg.preset("base")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", TRAINING_LEARNING_RATE=1e-4,
               TRAINING_WEIGHT_DECAY=1e-2, TRAINING_VIT_OPERANDS=operands, **size)
    torch.manual_seed(42)
    model = NeuroEncoder(cfg)
    model.train()
    return model, size["TRAINING_VIT_INPUT_SIZE"]


def make_batch(B, S, seed=42):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, S, S, generator=g).cuda(), (torch.arange(B) % 2).cuda()


def timed(fn, n):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n          # ms per call


def bench_steps(a, B, operands):
    import torch
    from neurovit_amd.trainer import TrainStep
    steps = {}
    x = y = None
    for name, kw in VARIANTS:                   # a model of its own per variant: every variant trains from the same start
        model, S = make_model(operands)
        if x is None:
            x, y = make_batch(B, S)
        steps[name] = TrainStep(model, **kw)
        for _ in range(a.warmup):
            steps[name](x, y)
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in VARIANTS}
    for _ in range(a.rounds):
        for name, _ in VARIANTS:
            ms[name].append(timed(lambda: steps[name](x, y), a.steps))
    out = {"batch": B, "operands": operands, "steps": a.steps, "rounds": a.rounds, "unit": "steps/s (median of rounds; min .. max)"}
    med = {}
    for name, _ in VARIANTS:
        rates = sorted(1e3 / t for t in ms[name])
        med[name] = statistics.median(rates)
        out[name] = {"median": round(med[name], 2), "min": round(rates[0], 2), "max": round(rates[-1], 2), "path": steps[name].last_path,
                     "fuse_update": steps[name].last_fuse_update}
    out["fuse_update=0 vs default %"] = round(100.0 * (med["fuse_update=0"] / med["default"] - 1.0), 2)
    out["clip vs fuse_update=0 %"] = round(100.0 * (med["clip"] / med["fuse_update=0"] - 1.0), 2)
    out["last_grad_norm"] = float(steps["clip"].last_grad_norm)
    out["last_clip_coef"] = float(steps["clip"].last_clip_coef)
    print(json.dumps(out), flush=True)


def bench_kernels(a):
    """nv_grad_sumsq (both launches) and nv_loss_scale_check back to back over a ViT3D-base sized arena"""
    import torch
    from neurovit_amd import ops
    from neurovit_amd.optim import LossScaler
    count = a.elements
    g = torch.randn(count, device="cuda") * 1e-3
    st = torch.zeros(ops.GRAD_CLIP_FLOATS, device="cuda")
    sc = LossScaler("cuda")
    out = {"arena_elements": count, "byte_floor_us_fp32": round(byte_floor_us(count), 1), "byte_floor_us_16bit": round(byte_floor_us(count, 2), 1),
           "unit": "us per call, device events around back-to-back calls (median of rounds; min .. max)"}
    cases = {"grad_sumsq fp32 (+ partials launch)": lambda: ops.grad_sumsq(g, st),
             "grad_sumsq fp32 + found_inf": lambda: ops.grad_sumsq(g, st, sc.state),
             "loss_scale_check": lambda: ops.loss_scale_check(g, sc.state)}
    g16 = g.to(ops.op16())
    cases["grad_sumsq 16-bit (+ partials launch)"] = lambda: ops.grad_sumsq(g16, st)
    for fn in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            us[k].append(1e3 * timed(fn, 50))
    for k in cases:
        v = sorted(us[k])
        out[k] = {"median": round(statistics.median(v), 1), "min": round(v[0], 1), "max": round(v[-1], 1)}
    out["grad_sumsq fp32 over byte floor"] = round(out["grad_sumsq fp32 (+ partials launch)"]["median"] / byte_floor_us(count), 3)
    out["grad_sumsq fp32 over loss_scale_check"] = round(out["grad_sumsq fp32 (+ partials launch)"]["median"] / out["loss_scale_check"]["median"], 3)
    print(json.dumps(out), flush=True)


def trace(a):
    import torch
    from neurovit_amd.trainer import TrainStep
    for operands in a.operands:
        model, S = make_model(operands)
        x, y = make_batch(a.batches[0], S)
        step = TrainStep(model, max_grad_norm=1.0)
        for _ in range(6):
            step(x, y)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--operands", nargs="+", default=["bf16", "fp16"], choices=["bf16", "fp16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--elements", type=int, default=88_580_000, help="gradient elements of the kernel timing (ViT3D-base: 88.58 M)")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--trace", action="store_true", help="a few clipped steps and nothing else: the program of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--stats", metavar="CSV", default=None, help="kernel_stats.csv of a --trace run: report the reduction kernel's duration")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats, a.elements)
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    if a.trace:
        return trace(a)
    if not a.no_kernels:
        bench_kernels(a)
    if not a.no_steps:
        for B in a.batches:
            for operands in a.operands:
                bench_steps(a, B, operands)


if __name__ == "__main__":
    main()
