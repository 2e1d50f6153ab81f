#!/usr/bin/env python3
"""Cost of stochastic depth (TRAINING_DROP_PATH; csrc/drop_path.hip and the path-aware residual sites) on the train step:

    step       TrainStep at TRAINING_DROP_PATH 0 (what the parent of this feature runs: without a rate the step makes exactly the calls it
               made) against 0.1, for ViT3D-base at batch 4 and batch 32 and the reference's 90^3 / patch 9 geometry at batch 32, in the
               current update mode (fuse_update = None: chosen by batch) and at fuse_update = 0
    draw       nv_drop_path_draw alone, depth 12, at the batches above

Everything is timed with device events around `--train-steps` / `--steps` repetitions; the two sides of every comparison take turns
(`--rounds` rounds each) and the median round is reported with its spread (median [min ... max]).  Dropped branches are still computed:
the step does not get cheaper with the rate.

    python tools/drop_path_bench.py
    python tools/drop_path_bench.py --only draw --steps 500

Prints one JSON line.
--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/drop_path_bench.py --only
draw` (a run of its own; tracing slows the host, so its event timings are not the ones to quote) and reports the draw kernel's OWN time.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="step,draw", help="comma-separated: step, draw")
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=200, help="repetitions inside one timed window of `draw`")
    ap.add_argument("--train-steps", type=int, default=20, help="train steps inside one timed window of `step`")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run with --only draw")
    args = ap.parse_args()
    if args.stats:
        rows = [r for r in csv.DictReader(open(args.stats)) if "drop_path_draw_kernel" in r["Name"]]
        calls, ns = sum(int(r["Calls"]) for r in rows), sum(float(r["TotalDurationNs"]) for r in rows)
        print(json.dumps({"kernel": "drop_path_draw_kernel", "calls": calls, "kernel_avg_us": round(ns / calls / 1e3, 2)}))
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

    def config(S, patch, rate):
        return dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_DROP_PATH=rate, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
                    GRADCAM_CUBE_SIZE=8 if S % 8 == 0 else 9, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2, GLOBAL_BASE_PATH="",
                    BEST_MODEL_PATH="", TRAINING_LEARNING_RATE=1e-4, TRAINING_WEIGHT_DECAY=1e-2, **BASE)

    what = [w for w in args.only.split(",") if w]
    result = {"rate": args.rate, "rounds": args.rounds}
    if "step" in what:
        result["step"] = {"train_steps": args.train_steps}
        for geo, B in CASES:
            S, patch = GEOMETRIES[geo]
            x = torch.randn(B, S, S, S, device="cuda")
            labels = torch.randint(0, 2, (B,), device="cuda")
            for mode in (None, 0):
                steps = {"rate_0": TrainStep(NeuroEncoder(config(S, patch, 0.0)).train(), fuse_update=mode),
                         "rate_on": TrainStep(NeuroEncoder(config(S, patch, args.rate)).train(), fuse_update=mode)}
                t = in_turns({k: (lambda s=s: s(x, labels)) for k, s in steps.items()}, args.train_steps)
                base = t["rate_0"]["median_us"]
                assert steps["rate_on"].last_path == "native" and steps["rate_on"]._vit.last_drop_path is not None
                result["step"][f"{geo}_batch_{B}_fuse_{'auto' if mode is None else mode}"] = dict(
                    t, fuse_update=steps["rate_0"].last_fuse_update, delta_us=round(t["rate_on"]["median_us"] - base, 1),
                    delta_share=round(t["rate_on"]["median_us"] / base - 1.0, 4), rate_0_volumes_per_s=round(B / base * 1e6, 1))
                del steps
                torch.cuda.empty_cache()
            del x
    if "draw" in what:
        result["draw"] = {"steps": args.steps, "depth": 12}
        for B in sorted({b for _, b in CASES}):
            out = torch.empty((12, 2, B), device="cuda")
            t = in_turns({"draw": lambda: ops.drop_path_draw(1234, B, 12, args.rate, "linear", out=out)}, args.steps)
            result["draw"][f"batch_{B}"] = t["draw"]
    print(json.dumps(result))


if __name__ == "__main__":
    main()
