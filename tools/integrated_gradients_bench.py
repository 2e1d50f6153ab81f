#!/usr/bin/env python3
"""Cost of native integrated gradients (NeuroEncoder.integrated_gradients), eval mode, frozen model, bf16 operands:

    native     one integrated_gradients(steps=--ig-steps, riemann_middle, zero baseline) call for the batch
    autograd   the loop of tests/test_input_grad_gpu.py::test_autograd_grad_and_integrated_gradients at the same steps and chunk: path points
               by stock tensor operations, one autograd graph per chunk, torch.autograd.grad, a stock weighted sum
    passes     the same number of plain graph-recording forward + data-only backward passes at the same chunk, from one static buffer
               (plus the one plain forward of cat(x, baseline))

native - passes is what the feature adds around the passes (points, score gradients, accumulation, finish, pooling); autograd - native is
what the stock route costs over it.  All are timed with device events around `steps` repetitions.

    python tools/integrated_gradients_bench.py --preset base --batch 4
    python tools/integrated_gradients_bench.py --preset reference --batch 32      # the reference's shipped config: 90^3, patch 9

Prints one JSON line.
--trace: `--steps` native calls, nothing timed, for `rocprofv3 --kernel-trace --stats -- python tools/integrated_gradients_bench.py --trace ...`;
--stats CSV (with the same --preset / --batch / --ig-steps / --steps): reads that run's kernel_stats.csv and reports the new kernels against
their byte floors at the achievable HBM rate, and the share of all kernel time spent in them.
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
PP_GROUP = 8           # jobs one workgroup of path_points_kernel serves from one read of x (csrc/path_attr.hip)
KERNELS = ("path_points_kernel", "class_score_grads_kernel", "path_accumulate_kernel", "path_finish_kernel", "attr_token_sums_kernel")


def config_of(preset):
    p = dict(PRESETS[preset])
    S, patch = p.pop("size"), p.pop("patch")
    cfg = dict(DEVICE="cuda:0", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=S, TRAINING_VIT_PATCH_SIZE=patch,
               GRADCAM_CUBE_SIZE=8, DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=S // 2,
               GLOBAL_BASE_PATH="", BEST_MODEL_PATH="")
    cfg.update(p)
    return cfg


def default_chunk(S):
    return max(1, min(64, 2 ** 29 // (4 * S ** 3)))


def byte_floors(S, B, K, chunk):
    """bytes each streaming kernel must move in one native call (V = S^3 floats per volume; a zero scalar baseline)"""
    V, J = S ** 3, B * K
    launches = -(-J // chunk)
    return {
        "path_points_kernel": 4.0 * V * (J + J / min(PP_GROUP, K)),             # J rows written, x read once per group of jobs
        "path_accumulate_kernel": 4.0 * V * (J + 2.0 * max(B, launches)),       # J rows read, acc read and written once per launch that meets it
        "path_finish_kernel": 4.0 * V * 3 * B,                                  # acc and x read, attr written
        "attr_token_sums_kernel": 4.0 * V * B,                                  # attr read
    }


def stats(path, S, B, K, chunk, calls_traced):
    """the new kernels' time from a rocprofv3 kernel_stats.csv of a --trace run of `calls_traced` native calls"""
    rows = list(csv.DictReader(open(path)))
    total_ns = sum(float(r["TotalDurationNs"]) for r in rows)
    floors = byte_floors(S, B, K, chunk)
    out, new_ns = {}, 0.0
    for name in KERNELS:
        sel = [r for r in rows if name in r["Name"]]
        calls, ns = sum(int(r["Calls"]) for r in sel), sum(float(r["TotalDurationNs"]) for r in sel)
        new_ns += ns
        if calls:
            out[name] = {"calls": calls, "avg_us": round(ns / calls / 1e3, 2), "total_ms": round(ns / 1e6, 3)}
            if name in floors:
                floor_ms = calls_traced * floors[name] / (HBM_TBS * 1e12) * 1e3
                out[name].update(floor_ms=round(floor_ms, 3), TBps=round(calls_traced * floors[name] / ns / 1e3, 2),
                                 fraction_of_achievable=round(floor_ms / (ns / 1e6), 3))
    out["all_kernels_ms"] = round(total_ns / 1e6, 3)
    out["new_kernels_share"] = round(new_ns / total_ns, 4) if total_ns else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="base", choices=sorted(PRESETS))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ig-steps", type=int, default=16, help="points on the path")
    ap.add_argument("--chunk", type=int, default=0, help="points per pass (0: the call's default)")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trace", action="store_true", help="`--steps` native calls, nothing timed (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of a --trace run with the same --preset / --batch / --ig-steps / --steps")
    args = ap.parse_args()
    cfg = config_of(args.preset)
    S, B, K = cfg["TRAINING_VIT_INPUT_SIZE"], args.batch, args.ig_steps
    chunk = min(args.chunk or default_chunk(S), B * K)
    if args.stats:
        print(json.dumps({"preset": args.preset, "batch": B, "ig_steps": K, "chunk": chunk, **stats(args.stats, S, B, K, chunk, args.steps)}))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.NeuroEncoder import NeuroEncoder, path_quadrature
    require_gpu()
    torch.manual_seed(0)
    model = NeuroEncoder(cfg).eval().requires_grad_(False)
    vit = model.volume_encoder.vit3d
    x = torch.randn(B, S, S, S, device="cuda")
    static = torch.randn(chunk, S, S, S, device="cuda")
    alphas, weights = (t.cuda() for t in path_quadrature("riemann_middle", K))
    target = torch.zeros(B, dtype=torch.long, device="cuda")
    J = B * K

    def native():
        return model.integrated_gradients(x, target=target, steps=K, method="riemann_middle", chunk=chunk)

    def autograd():
        # volume-major jobs in slices of `chunk`, as the native call takes them
        b_of = torch.arange(B, device="cuda").repeat_interleave(K)
        a_of, w_of = alphas.repeat(B), weights.repeat(B)
        acc = torch.zeros_like(x)
        for first in range(0, J, chunk):
            sel = slice(first, min(first + chunk, J))
            path = (a_of[sel].view(-1, 1, 1, 1) * x[b_of[sel]]).requires_grad_(True)
            (g,) = torch.autograd.grad(model(path)[:, 0].sum(), path)
            acc.index_add_(0, b_of[sel], w_of[sel].view(-1, 1, 1, 1) * g)
        with torch.no_grad():
            model(torch.cat([x, torch.zeros_like(x)]))
        return x * acc

    def passes():
        with torch.no_grad():
            model(torch.cat([x, torch.zeros_like(x)]))
            for first in range(0, J, chunk):
                count = min(chunk, J - first)
                video = static[:count].permute(0, 3, 1, 2).unsqueeze(1)
                logits = vit._run_forward(video, True, (None, 0, None))
                dvideo = torch.empty_like(video, memory_format=torch.preserve_format)
                vit._rt.backward(torch.ones_like(logits), vit._arena, vit._shadow, None, accumulate=False, dvideo=dvideo, weight_grads=False)

    if args.trace:
        for _ in range(args.steps):
            native()
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

    t_native, t_autograd, t_passes = timed(native), timed(autograd), timed(passes)
    floors = byte_floors(S, B, K, chunk)
    print(json.dumps({"preset": args.preset, "batch": B, "size": S, "ig_steps": K, "jobs": J, "chunk": chunk, "steps": args.steps,
                      "native_ms": round(t_native, 3), "autograd_ms": round(t_autograd, 3), "passes_ms": round(t_passes, 3),
                      "added_ms": round(t_native - t_passes, 3), "added_share": round((t_native - t_passes) / t_native, 4),
                      "autograd_over_native": round(t_autograd / t_native, 4),
                      "new_kernels_floor_ms": round(sum(floors.values()) / (HBM_TBS * 1e12) * 1e3, 3)}))


if __name__ == "__main__":
    main()
