#!/usr/bin/env python3
"""Cost of perturbation attribution (NeuroEncoder.perturbation_curves / occlusion_sensitivity), eval mode, bf16 operands:

    call       one perturbation_curves(steps=20) / occlusion_sensitivity() call for the batch
    forwards   the same number of plain forwards at the same chunk size, from one static buffer (plus the one forward of x itself)

The difference is what the feature adds around the forward: ranking, the masked copies, scores, areas.  Both are timed with device events
around `steps` repetitions.

    python tools/perturbation_bench.py --preset base --batch 4
    python tools/perturbation_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line.
--trace --what curves|occlusion: `--steps` calls, nothing timed, for `rocprofv3 --kernel-trace --stats -- python tools/perturbation_bench.py --trace ...`;
--stats CSV (with the same --preset / --batch / --what / --steps): reads that run's kernel_stats.csv and reports nv_mask_patches' kernel against its write
floor J S^3 4 bytes at the achievable HBM rate, and the share of all kernel time spent in the new kernels.
--group N: jobs one workgroup of nv_mask_patches serves from one read of x (nv_mask_patches_set_group; default 4).
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {
    "base": dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072),
    "reference": dict(size=90, patch=9),      # the transformer size the reference hard-codes: d1024, L6, h8, mlp 2048
}
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
CURVE_STEPS = 20
KERNELS = ("token_ranks_kernel", "mask_patches_kernel", "class_scores_kernel", "curve_auc_kernel", "occlusion_gather_kernel")


def config_of(preset):
    p = dict(PRESETS[preset])
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
               GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2,
               GLOBAL_BASE_PATH="", BEST_MODEL_PATH="")
    cfg.update(p)
    return cfg


def jobs_of(what, cfg, B):
    N = (cfg["TRAINING_VIT_INPUT_SIZE"] // cfg["TRAINING_VIT_PATCH_SIZE"]) ** 3
    return B * (2 * (CURVE_STEPS + 1) if what == "curves" else N)


def default_chunk(S):
    return max(1, min(64, 2 ** 30 // (4 * S ** 3)))


def write_floor_us(S, J):
    return 4.0 * J * S ** 3 / (HBM_TBS * 1e12) * 1e6


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--what", default="curves,occlusion", help="curves, occlusion or both (comma-separated)")
    ap.add_argument("--group", type=int, default=0, help="nv_mask_patches_set_group (0: the library's default)")
    ap.add_argument("--trace", action="store_true", help="`--steps` calls of --what, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run with the same --preset / --batch / --what / --steps")
    args = ap.parse_args()
    cfg = config_of(args.preset)
    S, B = cfg["TRAINING_VIT_INPUT_SIZE"], args.batch
    what = [w for w in args.what.split(",") if w]
    if args.stats:
        jobs_total = args.steps * sum(jobs_of(w, cfg, B) for w in what)
        print(json.dumps({"preset": args.preset, "batch": B, "what": what, "jobs_masked": jobs_total, **stats(args.stats, S, jobs_total)}))
        return

    import torch
    from neurovit_amd._cabi import lib, require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    require_gpu()
    if args.group:
        assert lib.nv_mask_patches_set_group(args.group) == 0
    torch.manual_seed(0)
    model = NeuroEncoder(cfg).eval().requires_grad_(False)
    x = torch.randn(B, S, S, S, device="cuda")
    N = (S // cfg["TRAINING_VIT_PATCH_SIZE"]) ** 3
    maps = torch.relu(torch.randn(B, N, device="cuda"))
    chunk = default_chunk(S)
    static = torch.randn(chunk, S, S, S, device="cuda")

    calls = {"curves": lambda: model.perturbation_curves(x, maps, steps=CURVE_STEPS), "occlusion": lambda: model.occlusion_sensitivity(x)}

    def forwards(J):
        with torch.no_grad():
            model(x)
            for first in range(0, J, chunk):
                model(static[:min(chunk, J - first)])

    if args.trace:
        for w in what:
            for _ in range(args.steps):
                calls[w]()
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "what": what, "calls_each": args.steps}))
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

    out = {"preset": args.preset, "batch": B, "size": S, "tokens": N, "chunk": chunk, "steps": args.steps, "mask_group": args.group or "default"}
    for w in what:
        J = jobs_of(w, cfg, B)
        t_call, t_fwd = timed(calls[w]), timed(lambda: forwards(J))
        out[w] = {"jobs": J, "call_ms": round(t_call, 3), "forwards_ms": round(t_fwd, 3), "added_ms": round(t_call - t_fwd, 3),
                  "added_share": round((t_call - t_fwd) / t_call, 4), "mask_write_floor_ms": round(write_floor_us(S, J) / 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
