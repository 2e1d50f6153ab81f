#!/usr/bin/env python3
"""Cost of the regression objective (TrainStep(objective="regression"); csrc/regression.hip and the head step's regression form) on the
train step:

    step       TrainStep with the regression objective (K = 1; mse and huber) against the classification step of the same tree, for
               ViT3D-base at batch 4 and batch 32 and the reference's 90^3 / patch 9 geometry at batch 32, bf16 operands, in the current
               update mode (fuse_update = None: chosen by batch)
    loss       nv_reg_loss alone and nv_reg_metrics_update alone at those batches, K = 1

Everything is timed with device events around `--train-steps` / `--steps` repetitions; the sides of every comparison take turns
(`--rounds` rounds each) and the median round is reported with its spread (median [min ... max]).  The head step is two small launches
under either objective: no difference beyond the run-to-run spread is expected.

    python tools/regression_bench.py
    python tools/regression_bench.py --only loss --steps 500

Prints one JSON line.
--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/regression_bench.py --only
step --cases 0 --losses huber --rounds 1` (a run of its own; tracing slows the host, so its event timings are not the ones to quote) and
reports the OWN time of the head step's kernels: head_rows_kernel (classification) beside head_rows_reg_kernel, and head_sums_kernel.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = dict(TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072)
GEOMETRIES = {"base_128_p16": (128, 16), "base_90_p9": (90, 9)}
CASES = [("base_128_p16", 4), ("base_128_p16", 32), ("base_90_p9", 32)]
MEAN, STD = 74.0, 8.0           # ADNI's age: 56 ... 96 years, median 74


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="step,loss", help="comma-separated: step, loss")
    ap.add_argument("--steps", type=int, default=200, help="repetitions inside one timed window of `loss`")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps inside one timed window of `step`")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="0,1,2", help="comma-separated indices into the step cases (0: base batch 4, 1: base batch 32, 2: 90^3 / p9 batch 32)")
    ap.add_argument("--losses", default="mse,huber", help="comma-separated regression losses of `step`")
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run with --only step")
    args = ap.parse_args()
    if args.stats:
        out = {}
        for r in csv.DictReader(open(args.stats)):
            for key in ("head_rows_kernel", "head_rows_reg_kernel", "head_sums_kernel", "reg_loss_kernel"):
                if key + "<" in r["Name"] or key + "(" in r["Name"] or r["Name"].endswith(key):
                    e = out.setdefault(r["Name"].split("(")[0].replace("void ", ""), {"calls": 0, "ns": 0.0})
                    e["calls"] += int(r["Calls"]); e["ns"] += float(r["TotalDurationNs"])
        print(json.dumps({k: {"calls": v["calls"], "kernel_avg_us": round(v["ns"] / v["calls"] / 1e3, 2)} for k, v in out.items()}))
        return

    import torch
    from neurovit_amd import ops
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
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

    def config(S, patch, regression):
        extra = dict(TRAINING_OBJECTIVE="regression", REGRESSION_TARGETS=1, REGRESSION_TARGET_MEAN=[MEAN], REGRESSION_TARGET_STD=[STD]) if regression else {}
        return dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
                    GRADCAM_CUBE_SIZE=8 if S % 8 == 0 else 9, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2, GLOBAL_BASE_PATH="",
                    BEST_MODEL_PATH="", TRAINING_LEARNING_RATE=1e-4, TRAINING_WEIGHT_DECAY=1e-2, **BASE, **extra)

    what = [w for w in args.only.split(",") if w]
    result = {"rounds": args.rounds}
    if "step" in what:
        result["step"] = {"train_steps": args.train_steps}
        for geo, B in [CASES[int(i)] for i in args.cases.split(",") if i]:
            S, patch = GEOMETRIES[geo]
            x = torch.randn(B, S, S, S, device="cuda")
            labels = torch.randint(0, 2, (B,), device="cuda")
            ages = MEAN + STD * torch.randn(B, device="cuda")
            reg = dict(objective="regression", target_mean=[MEAN], target_std=[STD])
            steps = {"classification": (TrainStep(NeuroEncoder(config(S, patch, False)).train()), labels)}
            for kind in [k for k in args.losses.split(",") if k]:
                steps[f"regression_{kind}"] = (TrainStep(NeuroEncoder(config(S, patch, True)).train(), regression_loss=kind, huber_delta=1.0, **reg), ages)
            t = in_turns({k: (lambda s=s, y=y: s(x, y)) for k, (s, y) in steps.items()}, args.train_steps)
            base = t["classification"]["median_us"]
            assert all(s.last_path == "native" for s, _ in steps.values())
            result["step"][f"{geo}_batch_{B}"] = dict(
                t, fuse_update=steps["classification"][0].last_fuse_update, classification_volumes_per_s=round(B / base * 1e6, 1),
                **{f"{k}_delta_share": round(t[k]["median_us"] / base - 1.0, 4) for k in t if k != "classification"})
            del steps
            torch.cuda.empty_cache()
            del x
    if "loss" in what:
        result["loss"] = {"steps": args.steps}
        mean, std = torch.tensor([MEAN], device="cuda"), torch.tensor([STD], device="cuda")
        opts = ops.reg_opts("huber", 1.0, mean, std)
        for B in sorted({b for _, b in CASES}):
            z, y = torch.randn(B, 1, device="cuda"), MEAN + STD * torch.randn(B, 1, device="cuda")
            met = ops.RegressionMetrics(1, mean, std, "cuda")
            t = in_turns({"reg_loss": lambda: ops.reg_loss(z, y, opts), "metrics_update": lambda: met.update(z, y)}, args.steps)
            result["loss"][f"batch_{B}"] = t
    print(json.dumps(result))


if __name__ == "__main__":
    main()
