#!/usr/bin/env python3
"""Cost of Shapley value sampling (NeuroEncoder.shapley_values), eval mode, bf16 operands:

    call       one shapley_values(window=2, permutations=16) call for the batch
    forwards   the same number of plain forwards at the same chunk size, from one static buffer (plus the one forward of x itself)

The difference is what the feature adds around the forward: the draw, the label rows, the masked copies, the scores, the accumulator.
Both are timed with device events around `steps` repetitions.

    python tools/shapley_bench.py --preset base --batch 4
    python tools/shapley_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line.
--trace: `--steps` calls, nothing timed, for `rocprofv3 --kernel-trace --stats -- python tools/shapley_bench.py --trace ...`;
--stats CSV (with the same --preset / --batch / --steps): reads that run's kernel_stats.csv and reports the new kernels' own times, the masked
copies against their write floor J S^3 4 bytes at the achievable HBM rate, and the share of all kernel time spent in the new kernels;
--mask-ab: nv_mask_patches_rows against nv_mask_patches on the curve job table of tools/perturbation_bench.py (the same jobs with row = b),
side by side in alternating rounds: median [min ... max] of the per-launch time over the rounds.
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from perturbation_bench import CURVE_STEPS, PRESETS, config_of, default_chunk, write_floor_us  # noqa: E402

WINDOW, PERMUTATIONS = 2, 16
KERNELS = ("shapley_ranks_kernel", "shapley_labels_kernel", "mask_patches_kernel", "class_scores_kernel", "shapley_accumulate_kernel",
           "shapley_delta_kernel", "shapley_token_maps_kernel")


def players_of(cfg):
    G = cfg["TRAINING_VIT_INPUT_SIZE"] // cfg["TRAINING_VIT_PATCH_SIZE"]
    return (-(-G // WINDOW)) ** 3


def jobs_of(cfg, B):
    return B * (2 + PERMUTATIONS * (players_of(cfg) - 1))


def stats(path, S, jobs_total):
    """the new kernels' time from a rocprofv3 kernel_stats.csv of a --trace run that masked `jobs_total` copies"""
    rows = list(csv.DictReader(open(path)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    out, new_ns = {}, 0.0
    for name in KERNELS:
        sel = [r for r in rows if name in r["Name"]]
        calls, ns = sum(int(r["Calls"]) for r in sel), sum(float(r["TotalDurationNs"]) for r in sel)
        new_ns += ns
        if calls:
            out[name] = {"calls": calls, "avg_us": round(ns / calls / 1e3, 2), "total_ms": round(ns / 1e6, 3)}
            if name == "mask_patches_kernel":
                floor_ms = write_floor_us(S, jobs_total) / 1e3
                out["mask_write_floor_ms"] = round(floor_ms, 3)
                out["mask_write_TBps"] = round(4.0 * jobs_total * S ** 3 / ns / 1e3, 2)
                out["mask_fraction_of_achievable"] = round(floor_ms / (ns / 1e6), 3)
    out["all_kernels_ms"] = round(total_ns / 1e6, 3)
    out["new_kernels_share"] = round(new_ns / total_ns, 4) if total_ns else None
    return out


def spread(values):
    v = sorted(values)
    mid = v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    return {"median_us": round(mid, 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}


def mask_ab(cfg, B, rounds, reps):
    """the curve job table of perturbation_bench through both entry points, chunk by chunk as the methods call them"""
    import torch
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import perturbation_step_bounds
    S, p = cfg["TRAINING_VIT_INPUT_SIZE"], cfg["TRAINING_VIT_PATCH_SIZE"]
    N = (S // p) ** 3
    x = torch.randn(B, S, S, S, device="cuda")
    labels = ops.token_ranks(torch.relu(torch.randn(B, N, device="cuda")))
    m = perturbation_step_bounds(N, CURVE_STEPS).tolist()
    rows = []
    for b in range(B):
        rows += [(b, 0, m[k]) for k in range(CURVE_STEPS + 1)] + [(b, m[k], N) for k in range(CURVE_STEPS + 1)]
    jobs3 = torch.tensor(rows, dtype=torch.int32, device="cuda")
    jobs4 = torch.stack([jobs3[:, 0], jobs3[:, 0], jobs3[:, 1], jobs3[:, 2]], 1).contiguous()
    chunk = default_chunk(S)
    out = torch.empty((min(chunk, jobs3.shape[0]), S, S, S), device="cuda")
    slices = [(first, min(chunk, jobs3.shape[0] - first)) for first in range(0, jobs3.shape[0], chunk)]

    def run(fn, jobs):
        for first, count in slices:
            fn(x, labels, jobs[first:first + count], p, out=out[:count])

    def timed(fn, jobs):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(reps):
            run(fn, jobs)
        end.record()
        torch.cuda.synchronize()
        return begin.elapsed_time(end) * 1e3 / (reps * len(slices))
    run(ops.mask_patches, jobs3)
    run(ops.mask_patches_rows, jobs4)
    a, b4 = [], []
    for _ in range(rounds):                                    # alternating: drift of the clocks lands on both
        a.append(timed(ops.mask_patches, jobs3))
        b4.append(timed(ops.mask_patches_rows, jobs4))
    return {"jobs": jobs3.shape[0], "launches": len(slices), "rounds": rounds, "write_floor_us_per_launch": round(write_floor_us(S, jobs3.shape[0]) / len(slices), 2),
            "nv_mask_patches": spread(a), "nv_mask_patches_rows": spread(b4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true", help="`--steps` calls, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run with the same --preset / --batch / --steps")
    ap.add_argument("--mask-ab", action="store_true", help="nv_mask_patches_rows against nv_mask_patches on the curve job table")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    cfg = config_of(args.preset)
    S, B = cfg["TRAINING_VIT_INPUT_SIZE"], args.batch
    J = jobs_of(cfg, B)
    if args.stats:
        print(json.dumps({"preset": args.preset, "batch": B, "jobs_masked": args.steps * J, **stats(args.stats, S, args.steps * J)}))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    require_gpu()
    if args.mask_ab:
        print(json.dumps({"preset": args.preset, "batch": B, "size": S, "mask_ab": mask_ab(cfg, B, args.rounds, args.reps)}))
        return
    torch.manual_seed(0)
    model = NeuroEncoder(cfg).eval().requires_grad_(False)
    x = torch.randn(B, S, S, S, device="cuda")
    chunk = default_chunk(S)
    static = torch.randn(chunk, S, S, S, device="cuda")

    def call():
        return model.shapley_values(x, window=WINDOW, permutations=PERMUTATIONS)

    def forwards():
        with torch.no_grad():
            model(x)
            for first in range(0, J, chunk):
                model(static[:min(chunk, J - first)])

    if args.trace:
        for _ in range(args.steps):
            call()
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "calls": args.steps}))
        return

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.steps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return begin.elapsed_time(end) / args.steps

    t_call, t_fwd = timed(call), timed(forwards)
    print(json.dumps({"preset": args.preset, "batch": B, "size": S, "players": players_of(cfg), "permutations": PERMUTATIONS, "window": WINDOW, "chunk": chunk,
                      "steps": args.steps, "jobs": J, "call_ms": round(t_call, 3), "forwards_ms": round(t_fwd, 3), "added_ms": round(t_call - t_fwd, 3),
                      "added_share": round((t_call - t_fwd) / t_call, 4), "mask_write_floor_ms": round(write_floor_us(S, J) / 1e3, 3)}))


if __name__ == "__main__":
    main()
