#!/usr/bin/env python3
"""Cost of the permutation test (csrc/perm_test.hip; neurovit_amd.stats) at the shapes it was built for:

    validation cohort, exhaustive   N = 17,  R = 2^17 sign flips, V = 90^3
    training cohort                 N = 160, R = 10 000,          V = 90^3
    patch grid                      N = 160, R = 10 000,          V = 1000

Sides: `native` = nv_perm_stats + nv_perm_maxstat + nv_perm_finish (the design matrix is given to both sides), `native_maxstat` = the hot
kernel alone, `torch_chunked` = the stock-torch route on the same device - ((M @ X[:, chunk]) - a) * c, clamp, abs, amax and the comparisons,
the chunk sized to a fixed temporary (--temp-mib), then the FWE counts from a sort of the maxima - and the fp32 MFMA time
2 R Npad V / 155 TFLOP/s.  The agreement of the two routes' counts is reported (torch's GEMM accumulates in another order, so near-ties may
fall on the other side).

Everything is timed with device events; the sides take turns (`--rounds` rounds each) and the median round is reported with its spread
(median [min ... max]).  Prints one JSON line.

    python tools/perm_test_bench.py
    python tools/perm_test_bench.py --shapes 2 --rounds 5

--stats CSV: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/perm_test_bench.py
--native-only --rounds 1` (a run of its own) and reports the own time of every perm_* kernel.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(17, 1 << 17, 90 ** 3, True), (160, 10000, 90 ** 3, False), (160, 10000, 1000, False)]
FP32_MFMA_TFLOPS = 155.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="0,1,2", help="comma-separated indices into the shapes")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per side, taken in turns")
    ap.add_argument("--steps", type=int, default=1, help="repetitions inside one timed window")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--temp-mib", type=int, default=1024, help="size of the [R, chunk] temporary of the torch route")
    ap.add_argument("--splits", type=int, default=0, help="row splits of nv_perm_maxstat (0 = automatic)")
    ap.add_argument("--native-only", action="store_true", help="time the native calls alone (for a traced run)")
    ap.add_argument("--stats", help="kernel_stats.csv of a traced run")
    args = ap.parse_args()
    if args.stats:
        out = {}
        for r in csv.DictReader(open(args.stats)):
            m = re.search(r"perm_\w+_kernel", r["Name"])
            if m:
                name = m.group(0)
                e = out.setdefault(name, {"calls": 0, "ns": 0.0})
                e["calls"] += int(r["Calls"]); e["ns"] += float(r["TotalDurationNs"])
        print(json.dumps({k: {"calls": v["calls"], "kernel_avg_us": round(v["ns"] / v["calls"] / 1e3, 2)} for k, v in out.items()}))
        return

    import torch
    from neurovit_amd import stats
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
        return {k: dict(median_us=round(statistics.median(v), 1), min_us=round(min(v), 1), max_us=round(max(v), 1)) for k, v in times.items()}

    result = {"rounds": args.rounds, "steps": args.steps, "temp_mib": args.temp_mib, "shapes": {}}
    for N, R, V, exact in [SHAPES[int(i)] for i in args.shapes.split(",") if i]:
        X = torch.randn(N, V, device="cuda")
        X[:, : V // 100] += 0.5
        M = stats.perm_design("one_sample", N, R, exact=exact, seed=1)
        ws = stats.perm_workspace(R, V, args.splits)
        st = stats.perm_stats(X, "one_sample", ws)
        a, c = st["a"], st["c"]
        out = {}

        def native():
            stats.perm_stats(X, "one_sample", ws, out=st)
            stats.perm_maxstat(X, M, a, c, ws, splits=args.splits)
            return stats.perm_finish("one_sample", N, R, V, c, ws, alphas=(0.05, 0.01), splits=args.splits, out=out)

        def maxstat():
            stats.perm_maxstat(X, M, a, c, ws, splits=args.splits)

        cols = max(64, (args.temp_mib << 20) // (4 * R))
        Mn = M[:, :N].contiguous()

        def stock():
            top = torch.full((R,), float("-inf"), device="cuda")
            s0 = torch.empty(V, device="cuda")
            cu = torch.empty(V, dtype=torch.int64, device="cuda")
            for b in range(0, V, cols):
                u = (((Mn @ X[:, b:b + cols]) - a[b:b + cols]) * c[b:b + cols]).clamp_(-1.0, 1.0).abs_()
                s0[b:b + cols] = u[0]
                cu[b:b + cols] = (u >= u[0]).sum(0)
                top = torch.maximum(top, u.amax(1))
            cf = R - torch.searchsorted(top.sort().values, s0, right=False)
            return cu, cf, top

        sides = {"native": native, "native_maxstat": maxstat} if args.native_only else {"native": native, "native_maxstat": maxstat, "torch_chunked": stock}
        t = in_turns(sides, args.steps)
        npad = (N + 3) & ~3
        floor_us = 2.0 * R * npad * V / (FP32_MFMA_TFLOPS * 1e12) * 1e6
        entry = dict(t, splits=lib.nv_perm_splits(R, V, args.splits), workspace_mib=round(ws.numel() / 2 ** 20, 1), mfma_floor_us=round(floor_us, 1),
                     maxstat_over_floor=round(t["native_maxstat"]["median_us"] / floor_us, 2), native_over_floor=round(t["native"]["median_us"] / floor_us, 2))
        if not args.native_only:
            res = native()
            cu, cf, top = stock()
            entry["torch_over_native"] = round(t["torch_chunked"]["median_us"] / t["native"]["median_us"], 2)
            entry["count_unc_agreement"] = round((res["count_unc"].long() == cu).float().mean().item(), 6)
            entry["count_fwe_agreement"] = round((res["count_fwe"].long() == cf).float().mean().item(), 6)
            entry["max_stat_difference"] = float((res["max_stat"] - top).abs().max().item())
            entry["voxels_fwe_below_0.05"] = int((res["p_fwe"] < 0.05).sum().item())
            del cu, cf, top
        result["shapes"][f"N{N}_R{R}_V{V}"] = entry
        del X, M, ws, st, a, c, out, Mn
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
