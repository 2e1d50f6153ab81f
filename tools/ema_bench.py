#!/usr/bin/env python3
"""Cost of the device-side weight average (neurovit_amd.ModelEma, csrc/ema.hip):

    kernel     nv_ema_update over an arena of ViT3D-base's size (88.58 M fp32 parameters), against
    torch      `ema_arena.lerp_(arena, w)` - the one stock launch that does the same job (not bit-defined: it may fuse the product)
    floor      12 bytes per parameter (two loads, one store) at the achievable HBM rate (6.3 TB/s)

and `step`: the ViT3D-base train step at batch 4 and batch 32 without an average (what the parent of this feature runs: with no
ema_decay the step makes exactly the calls it made), with TrainStep(ema_decay=0.9999) and with ema_update_every=4.  Everything is timed
with device events around `--steps` repetitions; the sides of every comparison take turns (`--rounds` rounds each) and the median round
is reported, with the spread.

    python tools/ema_bench.py                       # everything
    python tools/ema_bench.py --only kernel --steps 200

Prints one JSON line.
--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/ema_bench.py --only
kernel` (in a run of its own; tracing slows the host, so its event timings are not the ones to quote) and reports the kernel's OWN time
against the floor.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
BASE = dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072)
BASE_PARAMS = 88_580_000     # --stats only (no model is built there): ViT3D-base's arena, rounded


def floor_us(count):
    return 12.0 * count / (HBM_TBS * 1e12) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="kernel,step", help="comma-separated: kernel, step")
    ap.add_argument("--batches", default="4,32", help="comma-separated batch sizes of `step`")
    ap.add_argument("--steps", type=int, default=100, help="repetitions inside one timed window of `kernel`")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=20, help="train steps inside one timed window of `step`")
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run with --only kernel")
    args = ap.parse_args()
    if args.stats:
        rows = [r for r in csv.DictReader(open(args.stats)) if "ema_kernel" in r["Name"]]
        calls, ns = sum(int(r["Calls"]) for r in rows), sum(float(r["TotalDurationNs"]) for r in rows)
        fl = floor_us(BASE_PARAMS)
        print(json.dumps({"calls": calls, "kernel_avg_us": round(ns / calls / 1e3, 2), "floor_us": round(fl, 1), "share_of_floor": round(fl / (ns / calls / 1e3), 3)}))
        return

    import torch
    from neurovit_amd import ops
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.optim import ema_weight
    from neurovit_amd.trainer import TrainStep
    require_gpu()
    torch.manual_seed(0)

    def window(fn, reps):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return begin.elapsed_time(end) / reps * 1e3          # us

    def in_turns(sides, reps):
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                times[k].append(window(fn, reps))
        return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}

    p = dict(BASE)
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch, GRADCAM_CUBE_SIZE=8,
               DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2, GLOBAL_BASE_PATH="", BEST_MODEL_PATH="",
               TRAINING_LEARNING_RATE=1e-4, TRAINING_WEIGHT_DECAY=1e-2, **p)
    what = [w for w in args.only.split(",") if w]
    result = {"steps": args.steps, "rounds": args.rounds, "hbm_TBps": HBM_TBS}
    if "kernel" in what:
        count = NeuroEncoder(cfg).volume_encoder.vit3d.flat_parameters()[0].numel()
        arena, ema, lerp = torch.randn(count, device="cuda"), torch.randn(count, device="cuda"), torch.randn(count, device="cuda")
        w = ema_weight(0.9999)
        t = in_turns({"kernel": lambda: ops.ema_update(ema, arena, w), "torch": lambda: lerp.lerp_(arena, w)}, args.steps)
        fl = floor_us(count)
        result["kernel"] = {"parameters": count, "floor_us": round(fl, 1), "kernel": t["kernel"], "torch": t["torch"],
                            "kernel_share_of_floor": round(fl / t["kernel"]["median_us"], 3),
                            "kernel_TBps": round(12.0 * count / t["kernel"]["median_us"] / 1e6, 2),
                            "torch_over_kernel": round(t["torch"]["median_us"] / t["kernel"]["median_us"], 2)}
        del arena, ema, lerp
    if "step" in what:
        result["step"] = {}
        for B in [int(b) for b in args.batches.split(",") if b]:
            x = torch.randn(B, S, S, S, device="cuda")
            labels = torch.randint(0, 2, (B,), device="cuda")
            steps = {"plain": TrainStep(NeuroEncoder(cfg).train()), "ema": TrainStep(NeuroEncoder(cfg).train(), ema_decay=0.9999),
                     "ema_every_4": TrainStep(NeuroEncoder(cfg).train(), ema_decay=0.9999, ema_update_every=4)}
            t = in_turns({k: (lambda s=s: s(x, labels)) for k, s in steps.items()}, args.train_steps)
            base = t["plain"]["median_us"]
            result["step"][f"batch_{B}"] = dict(t, train_steps=args.train_steps, fuse_update=steps["plain"].last_fuse_update,
                                                ema_delta_us=round(t["ema"]["median_us"] - base, 1), ema_delta_share=round(t["ema"]["median_us"] / base - 1.0, 4),
                                                ema_every_4_delta_us=round(t["ema_every_4"]["median_us"] - base, 1),
                                                ema_every_4_delta_share=round(t["ema_every_4"]["median_us"] / base - 1.0, 4))
            del steps, x
            torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
