#!/usr/bin/env python3
"""Cost of the on-device classification metrics (ops.ClassificationMetrics; csrc/cls_metrics.hip):

    auc         nv_cls_auc (exact pair counting) at N = 8 680 and 78 820 rows, C = 2 and 5, against the stock-torch route on the device
                (per class: sort, average ranks of tied scores, the rank sum of the positives) and against its own integer-work floor:
                the kernel walks N^2 (row, row) pairs and spends at least 4 vector-ALU lane operations on each (two compares, two
                conditional adds), so floor = 4 N^2 / (256 CUs x 4 SIMDs x 16 lanes x --clock-ghz)
    update      nv_cls_metrics_update per call at B = 4 / 32 / 128 (C = 2, with the bank)
    validation  one validation pass of ViT3D-base (VALIDATION_PRECISION bf16, batch 4, 64 batches with subject names): the reference's pass
                (two .item() per batch) against VALIDATION_METRICS (one launch per batch, one host read per pass) - wall time around the
                pass with a device synchronisation at both ends, since what differs is host synchronisation

`auc` and `update` are timed with device events around `--steps` repetitions; the sides of every comparison take turns (`--rounds` rounds
each) and the median round is reported with its spread (median [min ... max]).

    python tools/cls_metrics_bench.py
    python tools/cls_metrics_bench.py --only auc --steps 20

Prints one JSON line.
--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/cls_metrics_bench.py --only
auc,update --rounds 1` (a run of its own; tracing slows the host, so its event timings are not the ones to quote) and reports the OWN time
of the kernels of cls_metrics.hip.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = dict(TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072)
KERNELS = ("cls_update_kernel", "cls_auc_kernel", "cls_auc_merge_kernel", "segment_labels_kernel", "cls_finish_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="auc,update,validation", help="comma-separated: auc, update, validation")
    ap.add_argument("--steps", type=int, default=20, help="repetitions inside one timed window of `auc`; `update` takes ten times as many")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", type=int, default=64, help="batches of 4 volumes in the validation pass")
    ap.add_argument("--clock-ghz", type=float, default=2.4, help="the engine clock the integer-work floor is counted at")
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run")
    args = ap.parse_args()
    if args.stats:
        out = {}
        for r in csv.DictReader(open(args.stats)):
            for key in KERNELS:
                if key in r["Name"]:
                    e = out.setdefault(key, {"calls": 0, "ns": 0.0})
                    e["calls"] += int(r["Calls"]); e["ns"] += float(r["TotalDurationNs"])
        print(json.dumps({k: {"calls": v["calls"], "kernel_avg_us": round(v["ns"] / v["calls"] / 1e3, 2)} for k, v in out.items()}))
        return

    import torch
    from neurovit_amd import ops
    from neurovit_amd._cabi import lib, require_gpu
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

    def spread(v):
        return dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2))

    def in_turns(sides, reps, timer=window):
        for fn in sides.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in sides}
        for _ in range(args.rounds):
            for k, fn in sides.items():
                times[k].append(timer(fn, reps))
        return {k: spread(v) for k, v in times.items()}

    def torch_auc(probs, labels, C):
        """the stock route on the device: per class a sort, the average rank of every run of tied scores, the positives' rank sum"""
        use = labels >= 0
        out = []
        for c in range(C):
            s, pos = probs[use, c], labels[use] == c
            _, inverse, counts = torch.unique(s, sorted=True, return_inverse=True, return_counts=True)
            last = torch.cumsum(counts, 0).double()                       # rank of the last member of each run (1-based)
            rank = (last - (counts.double() - 1.0) / 2.0)[inverse]
            n_pos = pos.sum().double()
            n_neg = use.sum().double() - n_pos
            out.append((rank[pos].sum() - n_pos * (n_pos + 1.0) / 2.0) / (n_pos * n_neg))
        return torch.stack(out)

    what = [w for w in args.only.split(",") if w]
    result = {"rounds": args.rounds}
    if "auc" in what:
        result["auc"] = {"steps": args.steps}
        for N in (8680, 78820):
            for C in (2, 5):
                probs = torch.softmax(2.0 * torch.randn(N, C, device="cuda"), dim=1)
                labels = torch.randint(0, C, (N,), dtype=torch.int32, device="cuda")
                native, stock = ops.cls_auc(probs, labels)[:, 0], torch_auc(probs, labels, C)
                agree = float((native - stock).abs().max())
                t = in_turns({"native": lambda: ops.cls_auc(probs, labels), "torch_sort": lambda: torch_auc(probs, labels, C)}, args.steps)
                floor = 4.0 * N * N / (256 * 4 * 16 * args.clock_ghz * 1e9) * 1e6
                result["auc"][f"N_{N}_C_{C}"] = dict(t, splits=lib.nv_cls_auc_splits(N, C, 0), floor_us=round(floor, 2), max_abs_difference=agree,
                                                      native_over_floor=round(t["native"]["median_us"] / floor, 2),
                                                      native_over_torch=round(t["native"]["median_us"] / t["torch_sort"]["median_us"], 3))
    if "update" in what:
        result["update"] = {"steps": 10 * args.steps}
        for B in (4, 32, 128):
            z, y = torch.randn(B, 2, device="cuda"), torch.randint(0, 2, (B,), dtype=torch.int32, device="cuda")
            met = ops.ClassificationMetrics(2, capacity=B)

            def update():
                met.size = 0
                met.update(z, y)
            result["update"][f"batch_{B}"] = in_turns({"update": update}, 10 * args.steps)
    if "validation" in what:
        from neurovit_amd.NeuroEncoder import NeuroEncoder
        from neurovit_amd.trainer import Trainer

        class Volumes(torch.utils.data.Dataset):
            """4 * batches items over eight stored volumes; four volumes per subject name"""

            def __init__(self, n):
                self.n, self.vol = n, torch.randn(8, 128, 128, 128)

            def __len__(self):
                return self.n

            def __getitem__(self, i):
                return f"sub-{i // 4:04d}", 0.0, self.vol[i % 8], (i // 4) % 2

        def config(**extra):
            return dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=128, TRAINING_VIT_PATCH_SIZE=16, GRADCAM_CUBE_SIZE=8,
                        DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=64, GLOBAL_BASE_PATH="", BEST_MODEL_PATH="",
                        TRAINING_LEARNING_RATE=1e-4, TRAINING_WEIGHT_DECAY=1e-2, GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=4,
                        TRAINING_NUM_WORKERS=0, VALIDATION_PRECISION="bf16", **BASE, **extra)
        data = Volumes(4 * args.batches)
        model = NeuroEncoder(config())
        sides = {"reference_pass": Trainer(config(), model, data, data), "validation_metrics": Trainer(config(VALIDATION_METRICS=True), model, data, data)}
        devnull = open(os.devnull, "w")

        def wall(fn, reps):
            torch.cuda.synchronize()
            begin = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - begin) / reps * 1e6            # us per pass

        def one_pass(t):
            stdout, sys.stdout = sys.stdout, devnull
            try:
                t._validation_pass(t.model, "", 0)
            finally:
                sys.stdout = stdout
        t = in_turns({k: (lambda tr=tr: one_pass(tr)) for k, tr in sides.items()}, 1, timer=wall)
        result["validation"] = dict(t, batches=args.batches, batch=4, per_batch_difference_us=round(
            (t["reference_pass"]["median_us"] - t["validation_metrics"]["median_us"]) / args.batches, 2))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
