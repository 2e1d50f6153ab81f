"""What tools/augment_bench.py, tools/affine_bench.py and tools/mix_bench.py share: the common command-line arguments, the byte floor, the
timing protocol - device events around `reps` repetitions, the sides of a comparison taking turns, the median round with its spread -
the report of a traced run's kernel_stats.csv, and the configuration of the ViT3D-base train step they all time."""
import argparse
import csv
import json
import statistics

HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
BASE = dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072)


def floor_us(B, S, T, reads=1):
    """the output written plus the source window read `reads` times, at the achievable HBM rate"""
    return (1 + reads) * 4.0 * B * S ** 3 * T / (HBM_TBS * 1e12) * 1e6


def parser(geometries, stats_help):
    """the arguments of the three tools; geometries: the names `--only` takes beside `step`"""
    names = [*geometries, "step"]
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(names), help="comma-separated: " + ", ".join(names))
    ap.add_argument("--steps", type=int, default=100, help="repetitions inside one timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=20, help="train steps inside one timed window of `step`")
    ap.add_argument("--stats", help=stats_help)
    return ap


def print_kernel_stats(path, kernel, head, floor):
    """the JSON line of `--stats`: the kernel's own average time in a traced run's kernel_stats.csv against the floor; head: the line's first fields"""
    rows = [r for r in csv.DictReader(open(path)) if kernel in r["Name"]]
    calls, ns = sum(int(r["Calls"]) for r in rows), sum(float(r["TotalDurationNs"]) for r in rows)
    print(json.dumps({**head, "calls": calls, "kernel_avg_us": round(ns / calls / 1e3, 2), "floor_us": round(floor, 1),
                      "share_of_floor": round(floor / (ns / calls / 1e3), 3)}))


def window(fn, reps):
    import torch
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / reps * 1e3          # us


def in_turns(sides, reps, args):
    """sides: {name: fn} -> {name: median / min / max us per call over args.rounds windows of `reps` calls, the sides taking turns}"""
    import torch
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():
            times[k].append(window(fn, reps))
    return {k: dict(median_us=round(statistics.median(v), 2), min_us=round(min(v), 2), max_us=round(max(v), 2)) for k, v in times.items()}


def base_step_config():
    """(config of the ViT3D-base NeuroEncoder whose train step the tools time, its input size)"""
    p = dict(BASE)
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch, GRADCAM_CUBE_SIZE=8,
               DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2, GLOBAL_BASE_PATH="", BEST_MODEL_PATH="",
               TRAINING_LEARNING_RATE=1e-4, TRAINING_WEIGHT_DECAY=1e-2, **p)
    return cfg, S
