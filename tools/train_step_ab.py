"""Same bits before and after a change to TrainStep / FusedAdamW: runs a list of TrainStep configurations on the tiny test model and dumps
losses, last logits, parameters, gradient arenas, AdamW moment arenas, the loss-scale block and the averaged model as raw bytes; a second
mode compares such dumps.  Touches only public constructor arguments and public methods (and reads how many captured graphs a step holds),
so the same script runs against two trees of the Python package that share one built library:

    python tools/train_step_ab.py run --tree <tree that holds neurovit_amd/> --out <dir>
    python tools/train_step_ab.py compare <dir parent run 1> <dir parent run 2> <dir branch> [--table FILE]
"""
import argparse
import os
import struct
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)


def fbits(v: float) -> int:
    return struct.unpack("<i", struct.pack("<f", v))[0]


def mix_table():
    """A VolumeMix table ([B, 12] int32: partner, mode, lambda bits, label lambda bits, tries, box[6], 0) for a batch of two"""
    rows = [[1, 1, fbits(0.3), fbits(0.3), 1, 0, 0, 0, 0, 0, 0, 0], [0, 1, fbits(0.9), fbits(0.9), 1, 0, 0, 0, 0, 0, 0, 0]]
    return torch.tensor(rows, dtype=torch.int32).cuda()


def model3d(W, operands=None, dropout=0.0):
    import neurovit_amd.NeuroEncoder as ne
    cfg = W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **SIZE)
    cfg["TRAINING_DROPOUT"] = dropout
    model = ne.NeuroEncoder(cfg)
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), 1, prefix="volume_encoder.vit3d."), strict=True)
    if operands is not None:
        model.set_operands(operands)
    model.train()
    return model


def model4d(W):
    """NeuroEncoder dim 4 on a two-block encoder, 16^3 x 8 timepoints: the general path with the temporal head's arena"""
    import neurovit_amd.NeuroEncoder as ne
    with tempfile.TemporaryDirectory() as td:
        torch.manual_seed(11)
        torch.save(ne.NeuroEncoder(W.neuro_config(16, 8, DEVICE="cuda", **SIZE)).state_dict(), os.path.join(td, "c.pth"))
        torch.manual_seed(12)
        model = ne.NeuroEncoder(W.neuro_config(16, 8, dim=4, DEVICE="cuda", GLOBAL_BASE_PATH=td, BEST_MODEL_PATH="c.pth", TRAINING_LEARNING_RATE=1e-2, **SIZE))
    model.train()
    model.volume_encoder.eval()
    return model


def data3d(W, seed):
    return W.make_volume((2, 32, 32, 32), seed).cuda(), (torch.arange(2) % 2).cuda()


def dump(step, model, losses) -> dict:
    opt = step.optimizer
    out = {"losses": torch.stack([l.reshape(()) for l in losses]), "logits": step.last_outputs,
           "parameters": torch.cat([p.detach().reshape(-1) for p in model.parameters()])}
    for i, holder in enumerate(opt.arenas()):
        m, v = opt.arena_state(holder)
        out[f"gradients{i}"], out[f"exp_avg{i}"], out[f"exp_avg_sq{i}"] = holder.flat_gradients(), m, v
    if step.scaler is not None:
        out["scaler"] = step.scaler.state
    if step.ema is not None:
        out["ema"] = torch.cat([p.detach().reshape(-1) for p in step.ema.module.parameters()])
    torch.cuda.synchronize()
    arrays = {k: t.detach().float().cpu().contiguous().numpy() for k, t in out.items()}
    arrays["path"] = np.array(f"{step.last_path}, fuse_update {step.last_fuse_update}, {len(getattr(step, '_graphs', {}))} graphs held")
    return arrays


def run_steps(step, batches, mix=None):
    losses = []
    for x, y in batches:
        losses.append((step(x, y) if mix is None else step(x, y, mix)).detach().clone())      # (a replayed graph overwrites its own output)
    return losses


def configurations(W):
    """(name, environment, function -> dump).  Three optimizer steps each unless the name says otherwise."""
    from neurovit_amd.optim import LRSchedule
    from neurovit_amd.trainer import TrainStep
    three = lambda: [data3d(W, s) for s in (7, 8, 9)]

    def plain(batches=None, operands=None, dropout=0.0, mix=None, **kw):
        def go():
            model = model3d(W, operands, dropout)
            step = TrainStep(model, **kw)
            return dump(step, model, run_steps(step, three() if batches is None else batches(), mix and mix_table()))
        return go

    def graphs():
        model = model3d(W)
        step = TrainStep(model)
        a, b = data3d(W, 7), data3d(W, 8)
        return dump(step, model, run_steps(step, [a, b] * 4))

    def four_d(**kw):
        def go():
            model = model4d(W)
            step = TrainStep(model, **kw)
            y = torch.tensor([0, 1, 1, 0], device="cuda")
            return dump(step, model, run_steps(step, [(W.make_volume((4, 16, 16, 16, 8), s).cuda(), y) for s in (13, 14, 15)]))
        return go

    def resume():
        kw = dict(ema_decay=0.9, no_decay=True, layer_decay=0.75, lr_schedule=LRSchedule(1e-3, 10, 2))
        model = model3d(W, "fp16")
        step = TrainStep(model, **kw)
        losses = run_steps(step, three())
        state, weights = step.state_dict(), {k: v.clone() for k, v in model.state_dict().items()}
        fresh = model3d(W, "fp16")
        fresh.load_state_dict(weights, strict=True)
        again = TrainStep(fresh, **kw)
        again.load_state_dict(state)
        return dump(again, fresh, losses + run_steps(again, [data3d(W, s) for s in (10, 11)]))

    yield from ((f"native fuse_update {k}", {}, plain(fuse_update=k)) for k in (0, 1, 2, 3))
    yield "accumulation_steps 2 (6 micro-steps)", {}, plain(lambda: [data3d(W, s) for s in range(7, 13)], accumulation_steps=2)
    yield "dropout 0.1", {}, plain(dropout=0.1)
    yield "NEUROVIT_GRAPH_STEP=1, 2 buffers, 8 steps", {"NEUROVIT_GRAPH_STEP": "1"}, graphs
    yield "fp16 operands, dynamic scale", {}, plain(operands="fp16")
    yield "static loss scale 4096", {}, plain(loss_scale=4096.0)
    yield "max_grad_norm 0.5", {}, plain(max_grad_norm=0.5)
    yield "no_decay, layer_decay 0.75, cosine", {}, plain(no_decay=True, layer_decay=0.75, lr_schedule=LRSchedule(1e-3, 10, 2))
    yield "ema_decay 0.9", {}, plain(ema_decay=0.9)
    yield "Mixup table, label smoothing 0.1", {}, plain(mix=True, label_smoothing=0.1)
    yield "NEUROVIT_FORCE_COMPUTE_STREAM=1", {"NEUROVIT_FORCE_COMPUTE_STREAM": "1"}, plain()
    yield "native_dp on one rank", {}, plain(native_dp=True, n_buckets=3)
    yield "general path (NEUROVIT_NATIVE_STEP=0)", {"NEUROVIT_NATIVE_STEP": "0"}, plain()
    yield "4D plain", {}, four_d()
    yield "4D max_grad_norm 0.5", {}, four_d(max_grad_norm=0.5)
    yield "fp16 + ema + groups: 3 steps, state round trip, 2 steps", {}, resume


def run(tree: str, out: str) -> None:
    sys.path[:0] = [os.path.abspath(tree), os.path.join(ROOT, "tests", "golden")]
    import weights as W
    from neurovit_amd import _cabi
    _cabi.require_gpu()
    os.makedirs(out, exist_ok=True)
    for i, (name, env, go) in enumerate(configurations(W)):
        os.environ.update(env)
        torch.manual_seed(1234)
        try:
            arrays = go()
        finally:
            for k in env:
                del os.environ[k]
            _cabi.set_operand_format("bf16")
        np.savez(os.path.join(out, f"{i:02d}.npz"), name=np.array(name), **arrays)
        print(f"{i:02d} {name}: {', '.join(sorted(arrays))}", flush=True)


def compare(parent1: str, parent2: str, branch: str, table) -> int:
    lines = [f"{'configuration':<58} {'array':<12} {'elements':>9}  {'parent-parent max|d|':>20}  {'branch-parent max|d|':>20}  bytes equal  finite"]
    worst, paths = 0, ["", "path of the last step, the same in all three runs:"]
    for f in sorted(os.listdir(parent1)):
        a, b, c = (np.load(os.path.join(d, f)) for d in (parent1, parent2, branch))
        assert set(a.files) == set(b.files) == set(c.files), (f, a.files, c.files)
        assert str(a["path"]) == str(b["path"]) == str(c["path"]), (f, str(a["path"]), str(c["path"]))
        paths.append(f"{str(a['name']):<58} {a['path']}")
        for k in sorted(set(a.files) - {"name", "path"}):
            dev = [float(np.nanmax(np.abs(a[k].astype(np.float64) - o[k].astype(np.float64)))) if a[k].size else 0.0 for o in (b, c)]
            same = a[k].tobytes() == c[k].tobytes() and a[k].tobytes() == b[k].tobytes()
            worst += not same
            lines.append(f"{str(a['name']):<58} {k:<12} {a[k].size:>9}  {dev[0]:>20.3g}  {dev[1]:>20.3g}  {'yes' if same else 'NO':<11}  {'yes' if np.isfinite(c[k]).all() else 'no'}")
    text = "\n".join(lines + paths)
    print(text)
    if table:
        with open(table, "w") as fh:
            fh.write(text + "\n")
    return 1 if worst else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    r = sub.add_parser("run")
    r.add_argument("--tree", default=ROOT)
    r.add_argument("--out", required=True)
    c = sub.add_parser("compare")
    c.add_argument("dirs", nargs=3)
    c.add_argument("--table")
    a = ap.parse_args()
    if a.mode == "run":
        run(a.tree, a.out)
    else:
        sys.exit(compare(*a.dirs, a.table))
