#!/usr/bin/env python3
"""Cost of the random affine augmentation (neurovit_amd.augment.VolumeAffine, csrc/affine.hip): rotation +-10 degrees per axis, zoom
0.9 .. 1.1, translation +-4 voxels, on top of the crop.  The protocol is that of tools/augment_bench.py.  Sides:

    affine     nv_affine_apply into a preallocated output under a drawn table (prob = 1: every sample is resampled)
    integer    the same call under the table of prob = 0: integer maps, the fast path (one load per cell / one 16-byte load per group)
    augment    nv_augment_apply on the same crop - the existing index-copy kernel: the baseline for what the resampling adds
    torch      F.affine_grid + F.grid_sample(align_corners=True) on the device with the same matrices (its theta is formed on the host
               ONCE, outside the timed window; a series is permuted to channels-first inside it, as a user would have to).  It must agree
               with the kernel within the first-order bound 2^-24 (4 R A + 8 V) per cell (tests/affine_ref.py states it)
    floor      (output written + source window read once) at the achievable HBM rate (6.3 TB/s)

for the geometries

    base       ViT3D-base, batch 4, 136^3 -> 128^3                floor 10.7 us
    reference  the reference's shipped config, batch 128, 90^3 -> 80^3     83 us
    series     4D, B = 1, T = 20, 136^3 -> 128^3                   53 us
    series2    4D, B = 2, T = 20, 136^3 -> 128^3                  107 us

and `step`: the ViT3D-base batch-4 train step behind VolumeAugment (crop) against the same step behind VolumeAffine, both on 136^3
batches.  Everything is timed with device events around `--steps` repetitions; the sides of every comparison take turns (`--rounds`
rounds each) and the median round is reported, with the spread.

    python tools/affine_bench.py                       # everything
    python tools/affine_bench.py --only base,series --steps 200

Prints one JSON line.
--stats CSV --only NAME: reads the kernel_stats.csv of `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/affine_bench.py
--only NAME --sides affine` (one geometry and one side per traced run; tracing slows the host, so its event timings are not the ones to
quote) and reports the kernel's OWN time against the floor.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from augment_timing import HBM_TBS, base_step_config, floor_us, in_turns, parser, print_kernel_stats  # noqa: E402 (beside this script)

GEOMETRIES = {"base": dict(B=4, X=136, S=128, T=1), "reference": dict(B=128, X=90, S=80, T=1), "series": dict(B=1, X=136, S=128, T=20),
              "series2": dict(B=2, X=136, S=128, T=20)}
OPTIONS = dict(rotate=(10, 10, 10), zoom=(0.9, 1.1), translate=(4, 4, 4))
SIDES = ("affine", "integer", "augment", "torch")


def maps_of(table):
    """the [B, 3, 4] maps of a table, float64 on the host"""
    import torch
    return table[:, :12].cpu().view(torch.float32).double().view(-1, 3, 4)


def theta_of(table, X, S):
    """F.affine_grid's theta [B, 3, 4] (align_corners=True: normalised coordinates, (W, H, D) = (z, y, x) order) for the table's maps
    output cell -> source voxel: n_a = 2 s_a / (X - 1) - 1 with s_a = sum_b M_ab i_b + m_a3 and i_b = (u_b + 1) (S - 1) / 2"""
    import torch
    m = maps_of(table)
    half = (S - 1) / 2.0
    lin = m[:, :, :3] * half * 2.0 / (X - 1)
    off = (m[:, :, :3].sum(dim=2) * half + m[:, :, 3]) * 2.0 / (X - 1) - 1.0
    theta = torch.cat([lin, off[:, :, None]], dim=2)
    return theta.flip(1)[:, :, [2, 1, 0, 3]].float()


def torch_affine(x, theta, S):
    """x [B, X, Y, Z(, T)] -> [B, S, S, S(, T)] by stock device ops"""
    import torch.nn.functional as F
    vol = x.permute(0, 4, 1, 2, 3) if x.dim() == 5 else x[:, None]
    grid = F.affine_grid(theta, (x.shape[0], vol.shape[1], S, S, S), align_corners=True)
    out = F.grid_sample(vol, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return out.permute(0, 2, 3, 4, 1) if x.dim() == 5 else out[:, 0]


def share_of_bound(got, want, x, table, S):
    """max over cells of |got - want| / (2^-24 (4 R A + 8 V)), A = sum_a (|M_a0| i + |M_a1| j + |M_a2| k + |m_a3|), on the device"""
    import torch
    m = maps_of(table).abs().to(x.device)
    R, V = (max(x.max().item(), 0.0) - min(x.min().item(), 0.0)), x.abs().max().item()
    idx = torch.arange(S, dtype=torch.float64, device=x.device)
    worst = 0.0
    for b in range(x.shape[0]):
        A = sum(m[b, a, 0] * idx[:, None, None] + m[b, a, 1] * idx[None, :, None] + m[b, a, 2] * idx[None, None, :] + m[b, a, 3] for a in range(3))
        limit = 2.0 ** -24 * (4.0 * R * A + 8.0 * V)
        err = (got[b].double() - want[b].double()).abs()
        err = err.amax(dim=-1) if err.dim() == 4 else err
        worst = max(worst, (err / limit).max().item())
    return worst


def main():
    ap = parser(GEOMETRIES, "kernel_stats.csv of a traced run with the same --only (one geometry)")
    ap.add_argument("--sides", default=",".join(SIDES), help="comma-separated: " + ", ".join(SIDES))
    args = ap.parse_args()
    if args.stats:
        g = GEOMETRIES[args.only]
        print_kernel_stats(args.stats, "affine_apply_kernel", {"geometry": args.only, **g}, floor_us(g["B"], g["S"], g["T"]))
        return

    import torch
    from neurovit_amd._cabi import require_gpu
    from neurovit_amd.augment import VolumeAffine, VolumeAugment
    require_gpu()
    torch.manual_seed(0)

    what = [w for w in args.only.split(",") if w]
    wanted = [s for s in args.sides.split(",") if s]
    result = {"steps": args.steps, "rounds": args.rounds, "hbm_TBps": HBM_TBS, "options": {k: list(v) for k, v in OPTIONS.items()}}
    for name in what:
        if name == "step":
            continue
        g = GEOMETRIES[name]
        B, X, S, T = g["B"], g["X"], g["S"], g["T"]
        x = torch.randn((B, X, X, X, T) if T > 1 else (B, X, X, X), device="cuda")
        aff = VolumeAffine((S, S, S), fill=0.0, seed=1, **OPTIONS)
        still = VolumeAffine((S, S, S), fill=0.0, seed=1, prob=0.0, **OPTIONS)
        aug = VolumeAugment((S, S, S), fill=0.0, seed=1)
        table, table0, rows = aff.params(B, 0, in_size=(X, X, X)), still.params(B, 0, in_size=(X, X, X)), aug.params(B, 0, in_size=(X, X, X))
        out = torch.empty((B, S, S, S, T) if T > 1 else (B, S, S, S), device="cuda")
        theta = theta_of(table, X, S).cuda()
        sides = {"affine": lambda: aff.apply(x, table, out=out), "integer": lambda: still.apply(x, table0, out=out),
                 "augment": lambda: aug.apply(x, rows, out=out), "torch": lambda: torch_affine(x, theta, S)}
        sides = {k: v for k, v in sides.items() if k in wanted}
        fl = floor_us(B, S, T)
        entry = {**g, "floor_us": round(fl, 1)}
        if "torch" in sides and "affine" in sides:
            share = share_of_bound(aff.apply(x, table), torch_affine(x, theta, S), x, table, S)
            entry.update(torch_share_of_bound=round(share, 4), torch_agrees=bool(share <= 1.0))
        t = in_turns(sides, args.steps, args)
        entry.update(t)
        for k in ("affine", "integer", "augment"):
            if k in t:
                entry[k + "_share_of_floor"] = round(fl / t[k]["median_us"], 3)
        if "affine" in t and "augment" in t:
            entry["affine_over_augment"] = round(t["affine"]["median_us"] / t["augment"]["median_us"], 2)
        if "affine" in t and "torch" in t:
            entry["torch_over_affine"] = round(t["torch"]["median_us"] / t["affine"]["median_us"], 2)
        result[name] = entry
        del x, out, sides
        torch.cuda.empty_cache()
    if "step" in what:
        from neurovit_amd.NeuroEncoder import NeuroEncoder
        from neurovit_amd.trainer import TrainStep
        cfg, S = base_step_config()
        model = NeuroEncoder(cfg).train()
        step = TrainStep(model)
        B, X = 4, 136
        big = torch.randn(B, X, X, X, device="cuda")
        labels = torch.randint(0, 2, (B,), device="cuda")
        aug, aff = VolumeAugment((S, S, S), seed=1), VolumeAffine((S, S, S), seed=1, **OPTIONS)
        t = in_turns({"augment": lambda: step(aug(big), labels), "affine": lambda: step(aff(big), labels)}, args.train_steps, args)
        result["step"] = {"batch": B, "input": X, "size": S, "train_steps": args.train_steps, "augment": t["augment"], "affine": t["affine"],
                          "delta_us": round(t["affine"]["median_us"] - t["augment"]["median_us"], 1),
                          "delta_share": round(t["affine"]["median_us"] / t["augment"]["median_us"] - 1.0, 4)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
