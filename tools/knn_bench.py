#!/usr/bin/env python3
"""Cost of the frozen-feature kNN probe (csrc/features.hip; neurovit_amd.features):

    topk       ops.knn_topk (nv_knn_topk: fused similarity + top-k, the Nq x Nb matrix never written) against the chunked stock-torch route
               `(Q[c] @ bank.T).topk(k)` - what a user would otherwise write - and against the fp32 MFMA floor 2 Nq Nb d / 155 TFLOP/s, at
               k = 20 on random unit-norm rows: the reference set's size (Nq 8 680, Nb 78 820, d 1024), ViT3D-base's d = 768 at that size,
               and a small bank (Nq 512, Nb 4 096, d 768).  The agreement of the two routes' indices is reported (torch.topk breaks ties its
               own way and its GEMM accumulates in another order, so near-ties may swap).
    vote       ops.knn_vote at those query counts (C = 2, softmax weights)
    features   ViT.forward_features (patch_mean, normalised, into a bank row) against the plain eval forward at the same batch (ViT3D-base, batch 4)

Everything is timed with device events around `--steps` repetitions; the sides of every comparison take turns (`--rounds` rounds each) and
the median round is reported with its spread (median [min ... max]).  Prints one JSON line.

    python tools/knn_bench.py
    python tools/knn_bench.py --only topk --shapes 2

--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/knn_bench.py --only topk
--shapes 0 --rounds 1 --native-only` (a run of its own) and reports the own time of knn_topk_kernel and knn_merge_kernel.
"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(8680, 78820, 1024), (8680, 78820, 768), (512, 4096, 768)]
K = 20
FP32_MFMA_TFLOPS = 155.0
BASE = dict(image_size=128, image_patch_size=16, frames=128, frame_patch_size=16, num_classes=2, dim=768, depth=12, heads=12, mlp_dim=3072,
            channels=1, dim_head=64, pool="cls")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="topk,vote,features", help="comma-separated: topk, vote, features")
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices into the top-k shapes")
    ap.add_argument("--steps", type=int, default=3, help="repetitions inside one timed window")
    ap.add_argument("--rounds", type=int, default=5, help="timed windows per side, taken in turns")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=1024, help="query rows per chunk of the torch route")
    ap.add_argument("--splits", type=int, default=0, help="split count of nv_knn_topk (0 = automatic)")
    ap.add_argument("--native-only", action="store_true", help="time the native call alone (for a traced run)")
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run with --only topk")
    args = ap.parse_args()
    if args.stats:
        out = {}
        for r in csv.DictReader(open(args.stats)):
            for key in ("knn_topk_kernel", "knn_merge_kernel"):
                if key in r["Name"]:
                    e = out.setdefault(key, {"calls": 0, "ns": 0.0})
                    e["calls"] += int(r["Calls"]); e["ns"] += float(r["TotalDurationNs"])
        print(json.dumps({k: {"calls": v["calls"], "kernel_avg_us": round(v["ns"] / v["calls"] / 1e3, 2)} for k, v in out.items()}))
        return

    import torch
    import torch.nn.functional as F
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

    what = [w for w in args.only.split(",") if w]
    result = {"rounds": args.rounds, "steps": args.steps, "k": K}
    if "topk" in what:
        result["topk"] = {}
        for Nq, Nb, d in [SHAPES[int(i)] for i in args.shapes.split(",") if i]:
            Q = F.normalize(torch.randn(Nq, d, device="cuda"), dim=1)
            bank = F.normalize(torch.randn(Nb, d, device="cuda"), dim=1)

            def native():
                return ops.knn_topk(Q, bank, K, splits=args.splits)

            def stock():
                parts = [(Q[c:c + args.chunk] @ bank.T).topk(K, dim=1) for c in range(0, Nq, args.chunk)]
                return torch.cat([p.indices for p in parts]), torch.cat([p.values for p in parts])

            sides = {"native": native} if args.native_only else {"native": native, "torch_chunked": stock}
            t = in_turns(sides, args.steps)
            floor_us = 2.0 * Nq * Nb * d / (FP32_MFMA_TFLOPS * 1e12) * 1e6
            entry = dict(t, splits=lib.nv_knn_topk_splits(Nq, Nb, args.splits), mfma_floor_us=round(floor_us, 1),
                         native_over_floor=round(t["native"]["median_us"] / floor_us, 2))
            if not args.native_only:
                idx, sim = native()
                tidx, tsim = stock()
                entry["torch_over_native"] = round(t["torch_chunked"]["median_us"] / t["native"]["median_us"], 2)
                entry["index_agreement"] = round((idx == tidx.to(torch.int32)).float().mean().item(), 6)
                entry["rows_with_the_same_neighbour_set"] = round((idx.sort(1).values == tidx.to(torch.int32).sort(1).values).all(1).float().mean().item(), 6)
                entry["max_sim_difference"] = float((sim - tsim).abs().max().item())
                del idx, sim, tidx, tsim
            result["topk"][f"Nq{Nq}_Nb{Nb}_d{d}"] = entry
            del Q, bank
            torch.cuda.empty_cache()
    if "vote" in what:
        result["vote"] = {}
        for Nq in sorted({s[0] for s in SHAPES}):
            Nb = 4096
            idx = torch.randint(0, Nb, (Nq, K), device="cuda", dtype=torch.int32)
            sim = torch.rand(Nq, K, device="cuda").sort(1, descending=True).values
            labels = torch.randint(0, 2, (Nb,), device="cuda", dtype=torch.int32)
            result["vote"][f"Nq{Nq}"] = in_turns({"knn_vote": lambda: ops.knn_vote(idx, sim, K, labels=labels, num_classes=2)}, 20 * args.steps)
    if "features" in what:
        from neurovit_amd.vit_3d import ViT
        model = ViT(**BASE).cuda().eval()
        B = 4
        x = torch.randn(B, 1, 128, 128, 128, device="cuda")
        bank = torch.zeros(64, BASE["dim"], device="cuda")

        def plain():
            with torch.no_grad():
                return model(x)

        t = in_turns({"eval_forward": plain,
                      "features_own_pool": lambda: model.forward_features(x, normalize=True, out=bank, row0=8),
                      "features_patch_mean": lambda: model.forward_features(x, pool="patch_mean", normalize=True, out=bank, row0=8)}, 10 * args.steps)
        base = t["eval_forward"]["median_us"]
        result["features"] = dict(t, batch=B, **{f"{k}_delta_share": round(t[k]["median_us"] / base - 1.0, 4) for k in t if k != "eval_forward"})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
