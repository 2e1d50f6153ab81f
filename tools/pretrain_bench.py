#!/usr/bin/env python3
"""Cost of one masked-pretraining step (neurovit_amd.MaskedPretrainStep) beside the supervised step at the same batch, bf16 operands:

    pretrain     MaskedPretrainStep(model)(x): mask draw, masked copy, forward of every row, decoder, nv_recon_loss, decoder and encoder
                 backward, one AdamW step over both arenas
    supervised   TrainStep(model, fuse_update=0)(x, labels): the labelled step with AdamW behind the backward pass

Two models of one config; the sides take turns over `--rounds` rounds of `--steps` steps each, every round timed with device events;
reported: the median round [min ... max] in ms per step.

    python tools/pretrain_bench.py --preset base --batch 4
    python tools/pretrain_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line.
--trace: `--steps` pretraining steps, nothing timed, for `rocprofv3 --kernel-trace --stats -- python tools/pretrain_bench.py --trace ...`;
--stats CSV (with the same --preset / --batch): reads that run's kernel_stats.csv and reports nv_recon_loss' kernel against its byte floor at
the achievable HBM rate - pred read on the masked rows, dpred written on all rows, the masked patches read once.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {
    "base": dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072),
    "reference": dict(size=90, patch=9),      # the transformer size the reference hard-codes: d1024, L6, h8, mlp 2048
}
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
MASK_RATIO = 0.6


def config_of(preset):
    p = dict(PRESETS[preset])
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
               GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2,
               GLOBAL_BASE_PATH="", BEST_MODEL_PATH="")
    cfg.update(p)
    return cfg


def recon_floor(cfg, B):
    """(bytes, microseconds at HBM_TBS) nv_recon_loss must move: pred fp32 on the masked rows, dpred 16-bit on all rows, the masked patches once"""
    S, p = cfg["TRAINING_VIT_INPUT_SIZE"], cfg["TRAINING_VIT_PATCH_SIZE"]
    N, P = (S // p) ** 3, p ** 3
    P8 = (P + 7) // 8 * 8
    m = min(max(int(MASK_RATIO * N + 0.5), 1), N - 1)
    nbytes = B * m * (4 * P8 + 4 * P) + B * (N + 1) * 2 * P8
    return nbytes, nbytes / (HBM_TBS * 1e12) * 1e6


def stats(path, cfg, B):
    rows = list(csv.DictReader(open(path)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for name in ("recon_loss_kernel", "recon_sum_kernel", "mim_labels_kernel", "mask_patches_kernel", "token_grad_seed_kernel"):
        sel = [r for r in rows if name in r["Name"]]
        calls, ns = sum(int(r["Calls"]) for r in sel), sum(float(r["TotalDurationNs"]) for r in sel)
        if calls:
            out[name] = {"calls": calls, "avg_us": round(ns / calls / 1e3, 2), "share_of_kernel_time": round(ns / total_ns, 5)}
    nbytes, floor_us = recon_floor(cfg, B)
    out["recon_floor_bytes"], out["recon_floor_us"] = nbytes, round(floor_us, 2)
    if "recon_loss_kernel" in out:
        out["recon_fraction_of_floor_rate"] = round(floor_us / out["recon_loss_kernel"]["avg_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true", help="`--steps` pretraining steps, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run with the same --preset / --batch")
    args = ap.parse_args()
    cfg = config_of(args.preset)
    S, B = cfg["TRAINING_VIT_INPUT_SIZE"], args.batch
    if args.stats:
        print(json.dumps({"preset": args.preset, "batch": B, **stats(args.stats, cfg, B)}))
        return

    import torch
    from neurovit_amd import MaskedPretrainStep
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    from neurovit_amd.trainer import TrainStep
    require_gpu()
    torch.manual_seed(0)
    x = torch.randn(B, S, S, S, device="cuda")
    y = torch.randint(0, 2, (B,), device="cuda")
    pre_model = NeuroEncoder(cfg).train()
    pretrain = MaskedPretrainStep(pre_model, mask_ratio=MASK_RATIO)
    sides = {"pretrain": lambda: pretrain(x)}
    if args.trace:
        for _ in range(args.warmup + args.steps):
            sides["pretrain"]()
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "steps": args.warmup + args.steps}))
        return
    sup_model = NeuroEncoder(cfg).train()
    supervised = TrainStep(sup_model, fuse_update=0)
    sides["supervised"] = lambda: supervised(x, y)

    def timed(fn):
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(args.steps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return begin.elapsed_time(end) / args.steps

    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(args.rounds):
        for k, fn in sides.items():          # the sides take turns: drift of the machine lands on both
            times[k].append(timed(fn))
    out = {"preset": args.preset, "batch": B, "size": S, "steps": args.steps, "rounds": args.rounds, "masked_patches": pretrain.masked_patches}
    for k, v in times.items():
        out[k + "_ms"] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["pretrain_over_supervised"] = round(out["pretrain_ms"]["median"] / out["supervised_ms"]["median"], 3)
    nbytes, floor_us = recon_floor(cfg, B)
    out["recon_floor_us"] = round(floor_us, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
