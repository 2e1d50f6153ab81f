#!/usr/bin/env python3
"""Cost of parameter groups in the fused AdamW and in the ViT3D-base train step, one MI355X.

The kernel: nv_adamw_step_grouped with the recipe's table for ViT3D-base (no weight decay on biases / LayerNorm / embeddings plus
layer_decay 0.75: 28 groups, 90 segments) against nv_adamw_step over the same 88.58 M-element arena, back to back, device
events, `--rounds` rounds with the two taking turns; both stated against the byte floor (30 B per parameter at 6.3 TB/s).

The step, bf16 operands, batch 4 and 32:

    default         TrainStep(model)                                        AdamW where the batch rule puts it (fuse_update 3 up to 4096 token rows)
    fuse_update=0   TrainStep(model, fuse_update=0)                         one AdamW launch behind the backward pass
    groups          TrainStep(model, no_decay=True, layer_decay=0.75)       that route, with the grouped launch
    schedule        TrainStep(model, lr_schedule=LRSchedule(...))           a schedule alone: every mode kept, one scalar changes per step

    python tools/param_groups_bench.py                          # everything; one JSON line for the kernels and one per batch
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/param_groups_bench.py --trace     # both kernels, nothing timed
    python tools/param_groups_bench.py --stats OUT/.../kernel_stats.csv                       # each kernel's own duration from that run
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
BYTES_PER_PARAM = 30                            # p, g, m, v read (16) + p, m, v and the 16-bit shadow written (14)
LAYER_DECAY, WEIGHT_DECAY = 0.75, 0.05
KERNELS = {"adamw": "adamw_kernel", "adamw_grouped": "adamw_grouped_kernel"}


def byte_floor_us(count):
    return count * BYTES_PER_PARAM / (HBM_TBS * 1e12) * 1e6


def stats(path):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for tag, name in KERNELS.items():
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            out[tag] = {"calls": calls, "mean_us": round(sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e3, 2)}
    if len(out) == 2:
        out["grouped over plain"] = round(out["adamw_grouped"]["mean_us"] / out["adamw"]["mean_us"], 4)
    print(json.dumps(out), flush=True)


def make_model():
    import torch
    from neurovit_amd import config as nvcfg
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    size = nvcfg.preset("base")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", TRAINING_LEARNING_RATE=1e-4,
               TRAINING_WEIGHT_DECAY=WEIGHT_DECAY, TRAINING_VIT_OPERANDS="bf16", **size)
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


def kernel_cases():
    """(arena size, table shape, {name: launch}) on the recipe's table of ViT3D-base: the model's own arena and shadow, random gradients"""
    import torch
    from neurovit_amd import ops, param_groups, set_group_lrs
    from neurovit_amd.optim import FusedAdamW
    model, _ = make_model()
    vit = model.volume_encoder.vit3d
    opt = FusedAdamW(param_groups(model, WEIGHT_DECAY, no_decay=True, layer_decay=LAYER_DECAY), lr=1e-4, model=model)
    set_group_lrs(opt, 1e-4)
    opt.arenas()
    info = opt._arena_groups[id(vit)]
    pairs = opt._arena_pairs(vit)[1]
    p, p16 = vit.flat_parameters()
    if p16 is None or p16.numel() != p.numel():
        p16 = torch.empty(p.numel(), dtype=ops.op16(), device=p.device)
    n = p.numel()
    g = torch.randn(n, device="cuda") * 1e-3
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    seg = ops.AdamwSegments(info["ends"], info["index"], len(pairs), n, p.device)
    lrs, wds = [a for a, _ in pairs], [b for _, b in pairs]
    shape = {"arena_elements": n, "groups": len(pairs), "distinct_pairs": len(set(pairs)), "segments": len(info["ends"]),
             "spans": -(-n // 2048), "spans_with_a_boundary": len({e // 2048 for e in info["ends"][:-1] if e % 2048})}
    cases = {"nv_adamw_step": lambda: ops.adamw_step(p.detach(), g, m, v, p16, 1, 1e-4, weight_decay=WEIGHT_DECAY),
             "nv_adamw_step_grouped": lambda: ops.adamw_step_grouped(p.detach(), g, m, v, p16, 1, seg, lrs, wds)}
    return shape, cases, (model, opt, seg)


def bench_kernels(a):
    import torch
    shape, cases, keep = kernel_cases()
    n = shape["arena_elements"]
    out = dict(shape, byte_floor_us=round(byte_floor_us(n), 1), unit="us per call, device events around 50 back-to-back calls (median of rounds; min .. max)")
    for fn in cases.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in cases}
    for _ in range(a.rounds):
        for k, fn in cases.items():
            us[k].append(1e3 * timed(fn, 50))
    for k in cases:
        vals = sorted(us[k])
        out[k] = {"median": round(statistics.median(vals), 1), "min": round(vals[0], 1), "max": round(vals[-1], 1),
                  "over_byte_floor": round(statistics.median(vals) / byte_floor_us(n), 3),
                  "TB/s": round(n * BYTES_PER_PARAM / (statistics.median(vals) * 1e-6) / 1e12, 2)}
    out["grouped over plain"] = round(out["nv_adamw_step_grouped"]["median"] / out["nv_adamw_step"]["median"], 4)
    print(json.dumps(out), flush=True)


def variants():
    from neurovit_amd import LRSchedule
    return (("default", {}), ("fuse_update=0", {"fuse_update": 0}), ("groups", {"no_decay": True, "layer_decay": LAYER_DECAY}),
            ("schedule", {"lr_schedule": LRSchedule(1e-4, 100000, 1000, "cosine", 1e-6)}))


def bench_steps(a, B):
    import torch
    from neurovit_amd.trainer import TrainStep
    steps = {}
    x = y = None
    names = [name for name, _ in variants()]
    for name, kw in variants():                 # a model of its own per variant: every variant trains from the same start
        model, S = make_model()
        if x is None:
            x, y = make_batch(B, S)
        steps[name] = TrainStep(model, **kw)
        for _ in range(a.warmup):
            steps[name](x, y)
    torch.cuda.synchronize()
    ms = {name: [] for name in names}
    for _ in range(a.rounds):
        for name in names:
            ms[name].append(timed(lambda: steps[name](x, y), a.steps))
    out = {"batch": B, "operands": "bf16", "steps": a.steps, "rounds": a.rounds, "unit": "steps/s (median of rounds; min .. max)"}
    med = {}
    for name in names:
        rates = sorted(1e3 / t for t in ms[name])
        med[name] = statistics.median(rates)
        out[name] = {"median": round(med[name], 2), "min": round(rates[0], 2), "max": round(rates[-1], 2), "ms_per_step": round(1e3 / med[name], 3),
                     "path": steps[name].last_path, "fuse_update": steps[name].last_fuse_update, "param_groups": len(steps[name].optimizer.param_groups)}
    out["fuse_update=0 vs default %"] = round(100.0 * (med["fuse_update=0"] / med["default"] - 1.0), 2)
    out["groups vs fuse_update=0 %"] = round(100.0 * (med["groups"] / med["fuse_update=0"] - 1.0), 2)
    out["groups vs default %"] = round(100.0 * (med["groups"] / med["default"] - 1.0), 2)
    out["schedule vs default %"] = round(100.0 * (med["schedule"] / med["default"] - 1.0), 2)
    print(json.dumps(out), flush=True)


def trace():
    import torch
    _, cases, keep = kernel_cases()
    for _ in range(3):                          # 60 calls of each kernel, in windows of 20 that take turns
        for fn in cases.values():
            for _ in range(20):
                fn()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--trace", action="store_true", help="both kernels a few times and nothing else: the program of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--stats", metavar="CSV", default=None, help="kernel_stats.csv of a --trace run: report each kernel's own duration")
    a = ap.parse_args()
    if a.stats is not None:
        return stats(a.stats)
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    if a.trace:
        return trace()
    if not a.no_kernels:
        bench_kernels(a)
    if not a.no_steps:
        for B in a.batches:
            bench_steps(a, B)


if __name__ == "__main__":
    main()
