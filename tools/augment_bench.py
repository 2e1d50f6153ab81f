#!/usr/bin/env python3
"""Cost of the on-device training augmentation (neurovit_amd.augment.VolumeAugment, csrc/augment.hip), crop + flips + intensity:

    kernel     nv_augment_apply into a preallocated output, parameters already on the device
    torch      the same transform with stock torch device ops: per-sample slice, flip, pad, multiply-add, then stack - what a user
               writes without the kernel (its parameters are read back to the host ONCE, outside the timed window)
    floor      output bytes read + output bytes written at the achievable HBM rate (6.3 TB/s)

for three geometries:

    base       ViT3D-base, batch 4, 136^3 -> 128^3            floor 10.7 us
    reference  the reference's shipped config, batch 128, 90^3 -> 80^3     83 us
    series     4D, B = 1, T = 20, 136^3 -> 128^3               53 us

and `step`: the ViT3D-base batch-4 train step fed dense 128^3 batches against the same step behind VolumeAugment (crop + flips) on 136^3
batches.  Everything is timed with device events around `--steps` repetitions; the two sides of every comparison take turns (`--rounds`
rounds each) and the median round is reported, with the spread.

    python tools/augment_bench.py                       # everything
    python tools/augment_bench.py --only base,series --steps 200

Prints one JSON line.
--stats CSV --only NAME: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/augment_bench.py
--only NAME` (one geometry per traced run; tracing slows the host, so its event timings are not the ones to quote) and reports the
kernel's OWN time against the floor - the event timings above include the gaps between back-to-back launches.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from augment_timing import HBM_TBS, base_step_config, floor_us, in_turns, parser, print_kernel_stats  # noqa: E402 (beside this script)

GEOMETRIES = {"base": dict(B=4, X=136, S=128, T=1), "reference": dict(B=128, X=90, S=80, T=1), "series": dict(B=1, X=136, S=128, T=20)}
OPTIONS = dict(flip_prob=(0.5, 0.5, 0.5), max_shift=(4, 4, 4), scale=(0.9, 1.1), shift=(-0.1, 0.1))


def torch_augment(x, rows, S, fill):
    """the transform of nv_augment_apply in stock device ops; rows: the parameter rows as host lists (floats for scale / shift)"""
    import torch
    import torch.nn.functional as F
    out = []
    for b, (ox, oy, oz, flips, scale, shift) in enumerate(rows):
        lo = [max(0, o) for o in (ox, oy, oz)]
        hi = [min(n, o + S) for n, o in zip(x.shape[1:4], (ox, oy, oz))]
        w = x[b, lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] * scale + shift
        pad = []
        for a in (2, 1, 0):                                  # F.pad takes the last axis first
            o = (ox, oy, oz)[a]
            pad += [lo[a] - o, o + S - hi[a]]
        if any(pad):
            w = F.pad(w, ([0, 0] if x.dim() == 5 else []) + pad, value=fill)
        axes = [a for a in range(3) if (flips >> a) & 1]
        out.append(torch.flip(w, axes) if axes else w)
    return torch.stack(out)


def main():
    args = parser(GEOMETRIES, "kernel_stats.csv of a traced run with the same --only (one geometry)").parse_args()
    if args.stats:
        g = GEOMETRIES[args.only]
        print_kernel_stats(args.stats, "augment_apply_kernel", {"geometry": args.only, **g}, floor_us(g["B"], g["S"], g["T"]))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.augment import VolumeAugment, center_window
    require_gpu()
    torch.manual_seed(0)

    what = [w for w in args.only.split(",") if w]
    result = {"steps": args.steps, "rounds": args.rounds, "hbm_TBps": HBM_TBS, "options": {k: list(v) for k, v in OPTIONS.items()}}
    for name in what:
        if name == "step":
            continue
        g = GEOMETRIES[name]
        B, X, S, T = g["B"], g["X"], g["S"], g["T"]
        x = torch.randn((B, X, X, X, T) if T > 1 else (B, X, X, X), device="cuda")
        aug = VolumeAugment((S, S, S), fill=0.0, seed=1, **OPTIONS)
        params = aug.params(B, 0, in_size=(X, X, X))
        out = torch.empty((B, S, S, S, T) if T > 1 else (B, S, S, S), device="cuda")
        host = params.cpu()
        rows = [(*r[:4].tolist(), r[4:5].view(torch.float32).item(), r[5:6].view(torch.float32).item()) for r in host]
        same = torch.allclose(aug.apply(x, params), torch_augment(x, rows, S, 0.0), rtol=0, atol=1e-6)      # (the torch form may fuse the multiply-add)
        t = in_turns({"kernel": lambda: aug.apply(x, params, out=out), "torch": lambda: torch_augment(x, rows, S, 0.0)}, args.steps, args)
        fl = floor_us(B, S, T)
        result[name] = {**g, "floor_us": round(fl, 1), "kernel": t["kernel"], "torch": t["torch"], "torch_agrees": bool(same),
                        "kernel_share_of_floor": round(fl / t["kernel"]["median_us"], 3),
                        "kernel_TBps": round(2 * 4.0 * B * S ** 3 * T / t["kernel"]["median_us"] / 1e6, 2),
                        "torch_over_kernel": round(t["torch"]["median_us"] / t["kernel"]["median_us"], 2)}
    if "step" in what:
        from neurovit_amd.NeuroEncoder import NeuroEncoder
        from neurovit_amd.trainer import TrainStep
        cfg, S = base_step_config()
        model = NeuroEncoder(cfg).train()
        step = TrainStep(model)
        B, X = 4, 136
        big = torch.randn(B, X, X, X, device="cuda")
        dense = center_window(big, (S, S, S)).contiguous()
        labels = torch.randint(0, 2, (B,), device="cuda")
        aug = VolumeAugment((S, S, S), flip_prob=(0.5, 0.5, 0.5), seed=1)
        t = in_turns({"plain": lambda: step(dense, labels), "augmented": lambda: step(aug(big), labels)}, args.train_steps, args)
        result["step"] = {"batch": B, "input": X, "size": S, "train_steps": args.train_steps, "plain": t["plain"], "augmented": t["augmented"],
                          "delta_us": round(t["augmented"]["median_us"] - t["plain"]["median_us"], 1),
                          "delta_share": round(t["augmented"]["median_us"] / t["plain"]["median_us"] - 1.0, 4)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
