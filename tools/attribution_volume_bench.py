#!/usr/bin/env python3
"""Cost of attribution volumes for a batch, per method (gradcam / rollout / relevance), eval mode, bf16 operands:

    loop      B single-volume calls of get_attention_map / get_attention_rollout / get_attention_relevance (results on the CPU: every call
              copies its G^3 map to the host, takes the percentile and upsamples there)
    batched   one NeuroEncoder.attribution_volumes call (results on the device: nv_gradcam_reduce_per_volume, nv_token_map_to_volume)

Each variant is timed by the wall clock around `steps` repetitions with ONE device synchronisation at its end.

    python tools/attribution_volume_bench.py --preset base --batch 4
    python tools/attribution_volume_bench.py --preset base --batch 32
    python tools/attribution_volume_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line: ms per batch of both variants and the speed-up, per method, and the write floor of the volumes.
--trace: a few batched calls per method, nothing timed, for `rocprofv3 --kernel-trace --stats -- python tools/attribution_volume_bench.py --trace`;
--stats CSV: reads that run's kernel_stats.csv and reports the new kernels' own time against the write floor B S^3 4 bytes at the
achievable HBM rate.
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {
    "base": dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072),
    "reference": dict(size=90, patch=9),      # the transformer size the reference hard-codes: d1024, L6, h8, mlp 2048
}
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
METHODS = ("gradcam", "rollout", "relevance")
KERNELS = {"threshold": "token_map_threshold_kernel", "upsample": "upsample_trilinear_kernel", "gradcam_per_volume": "gradcam_reduce_kernel"}      # (a --trace run launches it per volume only)


def config_of(preset):
    p = dict(PRESETS[preset])
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
               GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2,
               GLOBAL_BASE_PATH="", BEST_MODEL_PATH="")
    cfg.update(p)
    return cfg


def write_floor_us(S, B):
    return 4.0 * B * S ** 3 / (HBM_TBS * 1e12) * 1e6


def stats(path, S, B):
    """the new kernels' time from a rocprofv3 kernel_stats.csv of a --trace run"""
    rows = list(csv.DictReader(open(path)))
    out = {"write_floor_us": round(write_floor_us(S, B), 1), "volume_MB": round(4.0 * B * S ** 3 / 1e6, 1)}
    for tag, name in KERNELS.items():
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            us = sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e3
            out[f"{tag}_calls"], out[f"{tag}_avg_us"] = calls, round(us, 2)
            if tag == "upsample":
                out["upsample_write_TBps"] = round(4.0 * B * S ** 3 / us / 1e6, 2)
                out["upsample_fraction_of_achievable"] = round(write_floor_us(S, B) / us, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--trace", action="store_true", help="a few batched calls per method, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: report the new kernels' time and write rate")
    args = ap.parse_args()
    cfg = config_of(args.preset)
    S, B = cfg["TRAINING_VIT_INPUT_SIZE"], args.batch
    if args.stats:
        print(json.dumps({"preset": args.preset, "batch": B, **stats(args.stats, S, B)}))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    require_gpu()
    torch.manual_seed(0)
    model = NeuroEncoder(cfg).eval()           # trainable, as get_attention_map needs it (its backward goes through autograd)
    x = torch.randn(B, S, S, S, device="cuda")
    methods = [m for m in args.methods.split(",") if m]
    single = {"gradcam": model.get_attention_map, "rollout": model.get_attention_rollout, "relevance": model.get_attention_relevance}

    if args.trace:
        for m in methods:
            for _ in range(args.steps):
                model.attribution_volumes(x, method=m)
                model.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "steps_per_method": args.steps}))
        return

    def loop(m):
        return [single[m](x[b:b + 1]) for b in range(B)]

    def batched(m):
        return model.attribution_volumes(x, method=m)

    def timed(fn, m):
        for _ in range(args.warmup):
            fn(m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            fn(m)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    out = {"preset": args.preset, "batch": B, "size": S, "grid": S // cfg["TRAINING_VIT_PATCH_SIZE"], "steps": args.steps,
           "write_floor_us": round(write_floor_us(S, B), 1)}
    for m in methods:
        t_loop, t_new = timed(loop, m), timed(batched, m)
        out[f"{m}_loop_ms"], out[f"{m}_batched_ms"] = round(t_loop, 3), round(t_new, 3)
        out[f"{m}_speedup"] = round(t_loop / t_new, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
