#!/usr/bin/env python3
"""Cost of the 4D model's spatio-temporal attribution (NeuroEncoder.attribution_series), eval mode, bf16 operands, device events:

    call      one attribution_series call per method (gradcam / rollout / relevance), scope and layout "series"
    passes    the bare encoder passes that call contains, at the same chunk: the recording forwards (twice when B T > chunk) and the data-only
              backwards for gradcam / relevance, the exporting forwards for rollout - no head, no reduction, no volumes
    upsample  nv_series_map_to_volumes in layout "series" against the route it replaces - layout "frames" (the existing upsampling kernel)
              followed by permute(0, 2, 3, 4, 1).contiguous() - on the same maps, the two taking turns repetition by repetition

    python tools/series_attribution_bench.py --preset base --batch 1 --time-points 20
    python tools/series_attribution_bench.py --preset base --batch 4 --time-points 20
    python tools/series_attribution_bench.py --preset reference --batch 4 --time-points 20      # the reference's shipped geometry: 90^3, patch 9

Prints one JSON line: ms per call and per bare passes for every method, ms of the two upsampling routes, and the write floor
B T S^3 4 bytes at the achievable HBM rate.
--trace: a few calls of the two upsampling routes and of every method, nothing timed, for
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/series_attribution_bench.py --trace ...`; --stats CSV reads that run's kernel_stats.csv and
reports the kernels' own time against the write floor.  Counters, if wanted, are a run of their own (`rocprofv3 --pmc` without tracing).
"""
import argparse
import csv
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRESETS = {
    "base": dict(size=128, patch=16, TRAINING_VIT_DIM=768, TRAINING_VIT_DEPTH=12, TRAINING_VIT_HEADS=12, TRAINING_VIT_MLP_DIM=3072),
    "reference": dict(size=90, patch=9),      # the transformer size the reference hard-codes: d1024, L6, h8, mlp 2048
    "micro": dict(size=16, patch=8, TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256),
}
HBM_TBS = 6.3          # achievable HBM bandwidth of the MI355X (TB/s)
METHODS = ("gradcam", "rollout", "relevance")
KERNELS = {"series_threshold": "series_threshold_kernel", "series_upsample": "upsample_series_kernel", "frames_upsample": "upsample_trilinear_kernel",
           "gradcam_reduce": "gradcam_reduce_kernel", "leave_one_out": "leave_one_out_kernel", "grad_x_input": "grad_x_input_kernel"}


def configs(preset, workdir):
    p = dict(PRESETS[preset])
    S, patch = p.pop("size"), p.pop("patch")
    common = dict(TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch, GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni",
                  GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2, **p)
    three = dict(common, DEVICE="cpu", TRAINING_DIM=3, GLOBAL_BASE_PATH="", BEST_MODEL_PATH="")
    four = dict(common, DEVICE="cuda:0", TRAINING_DIM=4, GLOBAL_BASE_PATH=workdir, BEST_MODEL_PATH="encoder.pth")
    return three, four


def write_floor_us(S, V):
    return 4.0 * V * S ** 3 / (HBM_TBS * 1e12) * 1e6


def stats(path, S, V):
    """the kernels' time from a rocprofv3 kernel_stats.csv of a --trace run"""
    rows = list(csv.DictReader(open(path)))
    out = {"write_floor_us": round(write_floor_us(S, V), 1), "volume_MB": round(4.0 * V * S ** 3 / 1e6, 1)}
    for tag, name in KERNELS.items():
        sel = [r for r in rows if name in r["Name"]]
        calls = sum(int(r["Calls"]) for r in sel)
        if calls:
            us = sum(float(r["TotalDurationNs"]) for r in sel) / calls / 1e3
            out[f"{tag}_calls"], out[f"{tag}_avg_us"] = calls, round(us, 2)
            if tag == "series_upsample":
                out["series_upsample_write_TBps"] = round(4.0 * V * S ** 3 / us / 1e6, 2)
                out["series_upsample_fraction_of_achievable"] = round(write_floor_us(S, V) / us, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--time-points", type=int, default=20)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--methods", default=",".join(METHODS))
    ap.add_argument("--trace", action="store_true", help="a few calls of every route, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run: report the kernels' time and write rate")
    args = ap.parse_args()
    S = PRESETS[args.preset]["size"]
    B, T = args.batch, args.time_points
    V = B * T
    if args.stats is not None:
        print(json.dumps({"preset": args.preset, "batch": B, "time_points": T, **stats(args.stats, S, V)}))
        return

    import torch
    from neurovit_amd import ops
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    require_gpu()
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as workdir:
        three, four = configs(args.preset, workdir)
        torch.save(NeuroEncoder(three).state_dict(), os.path.join(workdir, "encoder.pth"))
        model = NeuroEncoder(four).eval()
    vit = model.volume_encoder.vit3d
    G = S // four["TRAINING_VIT_PATCH_SIZE"]
    x = torch.randn(B, S, S, S, T, device="cuda")
    video = x.movedim(-1, 1).reshape(V, S, S, S).permute(0, 3, 1, 2).unsqueeze(1)
    maps = torch.relu(torch.randn(B, T, G ** 3, device="cuda"))
    methods = [m for m in args.methods.split(",") if m]
    spans = [(first, min(args.chunk, V - first)) for first in range(0, V, args.chunk)]
    seeds = torch.randn(V, 2, device="cuda")
    layers = list(range(vit._cfg.depth))

    def call(m):
        return model.attribution_series(x, method=m, chunk=args.chunk)

    def passes(m):
        with torch.no_grad():
            if m == "rollout":
                for first, count in spans:
                    vit.attention_maps(video[first:first + count], head_fusion="mean")
                return
            if len(spans) > 1:
                for first, count in spans:
                    vit.recording_forward(video[first:first + count])
            for first, count in spans:
                vit.recording_forward(video[first:first + count])
                vit.data_backward(seeds[first:first + count], layers if m == "relevance" else None, "relevance")

    def series_route():
        return ops.series_maps_to_volumes(maps, G, S, scope="series", keep_percent=5, layout="series")

    def frames_route():
        return ops.series_maps_to_volumes(maps, G, S, scope="series", keep_percent=5, layout="frames").permute(0, 2, 3, 4, 1).contiguous()

    if args.trace:
        for _ in range(args.steps):
            series_route()
            frames_route()
        for m in methods:
            for _ in range(args.steps):
                call(m)
        model.temporal_importance(x)
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "steps_per_route": args.steps}))
        return

    def timed(fns):
        """ms per repetition of each function, the functions taking turns repetition by repetition (device events)"""
        for fn in fns:
            for _ in range(args.warmup):
                fn()
        total = [0.0] * len(fns)
        for _ in range(args.steps):
            for i, fn in enumerate(fns):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                total[i] += t0.elapsed_time(t1)
        return [t / args.steps for t in total]

    out = {"preset": args.preset, "batch": B, "time_points": T, "size": S, "grid": G, "chunk": args.chunk, "steps": args.steps,
           "write_floor_us": round(write_floor_us(S, V), 1), "volume_MB": round(4.0 * V * S ** 3 / 1e6, 1)}
    t_series, t_frames = timed([series_route, frames_route])
    out["upsample_series_ms"], out["upsample_frames_permute_ms"] = round(t_series, 4), round(t_frames, 4)
    out["upsample_speedup"] = round(t_frames / t_series, 2)
    for m in methods:
        t_call, t_passes = timed([lambda: call(m), lambda: passes(m)])
        out[f"{m}_call_ms"], out[f"{m}_passes_ms"] = round(t_call, 3), round(t_passes, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
