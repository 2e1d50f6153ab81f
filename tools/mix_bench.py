#!/usr/bin/env python3
"""Cost of Mixup / CutMix on the device (neurovit_amd.augment.VolumeMix, csrc/mix.hip for the draws, csrc/augment.hip for the pass), fused with the crop + flips + intensity of
VolumeAugment:

    kernel     nv_augment_mix into a preallocated output, both tables already on the device (ONE pass)
    torch      nv_augment_apply followed by the stock-torch mix - `lam * x + (1 - lam) * x.flip(0)` with a per-sample lambda for Mixup, a
               per-sample box assignment from `x.flip(0)` for CutMix - what a user writes behind VolumeAugment without the kernel (the
               mix table is read back to the host ONCE, outside the timed window)
    floor      bytes at the achievable HBM rate (6.3 TB/s): the output written plus the source read once (CutMix, mode 0) or twice (Mixup)

for the geometries of tools/augment_bench.py (base: ViT3D-base batch 4, 136^3 -> 128^3; reference: batch 128, 90^3 -> 80^3; series: B = 2,
T = 20, 136^3 -> 128^3 - a series needs a partner) under each of `mixup` and `cutmix` (every sample mixed), and `step`: the ViT3D-base
batch-4 train step behind VolumeAugment against the same step behind VolumeMix + label smoothing + class weights.  Everything is timed
with device events around `--steps` repetitions; the sides of every comparison take turns (`--rounds` rounds each) and the median round
is reported, with the spread.

    python tools/mix_bench.py                       # everything
    python tools/mix_bench.py --only base --modes mixup --steps 200

Prints one JSON line.
--stats CSV --only NAME --modes MODE: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/mix_bench.py --only NAME --modes MODE` (one geometry and one mode per traced run, in a run of its own; tracing slows the host, so
its event timings are not the ones to quote) and reports the kernel's OWN time against the floor.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from augment_timing import HBM_TBS, base_step_config, in_turns, parser, print_kernel_stats  # noqa: E402 (beside this script)
from augment_timing import floor_us as floor_of_reads  # noqa: E402 (beside this script)

GEOMETRIES = {"base": dict(B=4, X=136, S=128, T=1), "reference": dict(B=128, X=90, S=80, T=1), "series": dict(B=2, X=136, S=128, T=20)}
OPTIONS = dict(flip_prob=(0.5, 0.5, 0.5), max_shift=(4, 4, 4), scale=(0.9, 1.1), shift=(-0.1, 0.1))
MODES = {"mixup": dict(mixup_alpha=0.4), "cutmix": dict(cutmix_alpha=1.0)}


def floor_us(B, S, T, mode):
    """the output written plus the source read once (CutMix, mode 0) or twice (Mixup)"""
    return floor_of_reads(B, S, T, reads=2 if mode == "mixup" else 1)


def torch_mix(a, rows):
    """the stock-torch mix of an augmented batch a [B, S, S, S(, T)]; rows: the mix table as host lists (floats for the lambdas)"""
    import torch
    partner = a.flip(0)
    if all(r[1] == 1 for r in rows):
        lam = torch.tensor([r[2] for r in rows], device=a.device).view(-1, *([1] * (a.dim() - 1)))
        return lam * a + (1 - lam) * partner
    out = a.clone()
    for b, r in enumerate(rows):
        if r[1] == 2:
            x0, x1, y0, y1, z0, z1 = r[5:11]
            out[b, x0:x1, y0:y1, z0:z1] = partner[b, x0:x1, y0:y1, z0:z1]
        elif r[1] == 1:
            out[b] = r[2] * a[b] + (1 - r[2]) * partner[b]
    return out


def main():
    ap = parser(GEOMETRIES, "kernel_stats.csv of a traced run with the same --only and --modes (one geometry, one mode)")
    ap.add_argument("--modes", default="mixup,cutmix", help="comma-separated: mixup, cutmix")
    args = ap.parse_args()
    if args.stats:
        g = GEOMETRIES[args.only]
        print_kernel_stats(args.stats, "augment_mix_kernel", {"geometry": args.only, "mode": args.modes, **g}, floor_us(g["B"], g["S"], g["T"], args.modes))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.augment import VolumeAugment, VolumeMix
    require_gpu()
    torch.manual_seed(0)

    what = [w for w in args.only.split(",") if w]
    modes = [m for m in args.modes.split(",") if m]
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
        mid = torch.empty_like(out)
        result[name] = dict(g)
        for mode in modes:
            mixer = VolumeMix(seed=1, **MODES[mode])
            table = mixer.params(B, 0, (S, S, S))
            host = table.cpu()
            rows = [[*r[:2].tolist(), r[2:3].view(torch.float32).item(), r[3:4].view(torch.float32).item(), *r[4:].tolist()] for r in host]
            same = torch.allclose(mixer.apply(x, table, augment=aug, augment_params=params), torch_mix(aug.apply(x, params), rows), rtol=0, atol=1e-5)
            t = in_turns({"kernel": lambda: mixer.apply(x, table, augment=aug, augment_params=params, out=out),
                          "torch": lambda: torch_mix(aug.apply(x, params, out=mid), rows)}, args.steps, args)
            fl = floor_us(B, S, T, mode)
            result[name][mode] = {"floor_us": round(fl, 1), "kernel": t["kernel"], "torch": t["torch"], "torch_agrees": bool(same),
                                  "kernel_share_of_floor": round(fl / t["kernel"]["median_us"], 3),
                                  "torch_over_kernel": round(t["torch"]["median_us"] / t["kernel"]["median_us"], 2)}
    if "step" in what:
        from neurovit_amd.NeuroEncoder import NeuroEncoder
        from neurovit_amd.trainer import TrainStep
        cfg, S = base_step_config()
        B, X = 4, 136
        big = torch.randn(B, X, X, X, device="cuda")
        labels = torch.randint(0, 2, (B,), device="cuda")
        aug = VolumeAugment((S, S, S), flip_prob=(0.5, 0.5, 0.5), seed=1)
        mixer = VolumeMix(mixup_alpha=0.4, cutmix_alpha=1.0, seed=1)
        plain = TrainStep(NeuroEncoder(cfg).train())
        mixed = TrainStep(NeuroEncoder(cfg).train(), label_smoothing=0.1, class_weight=[0.5, 2.0])

        def mixed_step():
            batch = mixer(big, augment=aug)
            return mixed(batch, labels, mix=mixer.last_mix)
        t = in_turns({"augmented": lambda: plain(aug(big), labels), "mixed": mixed_step}, args.train_steps, args)
        result["step"] = {"batch": B, "input": X, "size": S, "train_steps": args.train_steps, "augmented": t["augmented"], "mixed": t["mixed"],
                          "delta_us": round(t["mixed"]["median_us"] - t["augmented"]["median_us"], 1),
                          "delta_share": round(t["mixed"]["median_us"] / t["augmented"]["median_us"] - 1.0, 4)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
