#!/usr/bin/env python3
"""A transcript of the Trainer shell (neurovit_amd.trainer.Trainer) over fixed seeds: what it prints, logs, reads back from the device, writes
and returns - for comparing two versions of the shell, which must agree word for word (the kernels and their order are the step's, not the
shell's: there is no tolerance).

    python tools/trainer_transcript.py --out new.json
    python tools/trainer_transcript.py --out parent.json --root /path/to/a/checkout/of/the/parent        # its neurovit_amd, this script
    diff parent.json new.json

One process, 32^3 volumes, patch 8, dim 128, depth 2, heads 2; 24 training and 8 validation volumes, batch 4, 2 epochs, no loader workers.
Scenarios: (a) supervised 7-tuples with dropout, accumulation, a weight average, clipping and Mixup; (b) supervised 6-tuples, plain;
(c) regression with the Huber loss, a weight average and Mixup - each followed by evaluate_samples and both probes on demand; (d) "mim"
with a cosine schedule and both probes every epoch, (d2) the same with two poolings; (e) TRAINING_SAVE_STATE for one epoch, then a fresh
Trainer with TRAINING_RESUME_FROM for the next.
Per scenario: stdout and the _log payloads without the duration (and with the run directory's time stamp blanked), the device-to-host reads
of every batch by phase (a batch begins at Trainer._unpack; what follows the last batch of a phase counts to it), the files written, a
SHA-256 of the final state_dict (and of the weight average's) and the return values of validate and evaluate_samples."""
import argparse
import contextlib
import hashlib
import io
import json
import os
import re
import sys
import tempfile

p = argparse.ArgumentParser()
p.add_argument("--out", required=True)
p.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose neurovit_amd is driven")
p.add_argument("--only", default=None, help="comma-separated scenario names")
args = p.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
OUT = os.path.abspath(args.out)

import torch  # noqa: E402

from neurovit_amd.NeuroEncoder import NeuroEncoder  # noqa: E402
from neurovit_amd.trainer import Trainer  # noqa: E402

READS = ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__")
STAMP = re.compile(r"\d{4}-\d{2}-\d{2}_\d{2}-\d{2}-\d{2}")
DURATION = re.compile(r"\t\| duration: [0-9.]+s")


class Volumes(torch.utils.data.Dataset):
    """n volumes in the ADNI order: 7-tuples (subject, _, volume, _, _, age, label) or the 4D loader's 6-tuples (subject, _, volume, _, _, label);
    two volumes per subject, the age a known function of a planted intensity"""

    def __init__(self, n, seed, six=False):
        g = torch.Generator().manual_seed(seed)
        pattern = torch.randn(32, 32, 32, generator=torch.Generator().manual_seed(99))
        a = torch.rand(n, generator=g) * 2 - 1
        self.x = a[:, None, None, None] * pattern + 0.3 * torch.randn(n, 32, 32, 32, generator=g)
        self.age, self.y, self.six = 70.0 + 8.0 * a, (a > 0).long(), six

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        head = (f"s{i // 2}", torch.tensor(0), self.x[i], torch.tensor(0), torch.tensor(1))
        return head + (self.y[i],) if self.six else head + (self.age[i], self.y[i])


def config(out_dir, **extra):
    cfg = dict(DEVICE="cuda", TRAINING_DIM=3, TRAINING_DROPOUT=0.0, TRAINING_VIT_INPUT_SIZE=32, TRAINING_VIT_PATCH_SIZE=8, GRADCAM_CUBE_SIZE=8,
               DATASET_NAME="adni", GRADCAM_THRESHOLD=5, GRADCAM_SLICE_DIM=2, GRADCAM_SLICE_IDX=16, GLOBAL_BASE_PATH="", BEST_MODEL_PATH="",
               TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256, TRAINING_LEARNING_RATE=1e-3,
               TRAINING_WEIGHT_DECAY=1e-2, PRETRAIN_LINEAR_STEPS=20, GLOBAL_OUTPUT_DIR=os.path.join(out_dir, "runs"), TRAINING_EPOCHS=2,
               TRAINING_BATCH_SIZE=4, TRAINING_NUM_WORKERS=0)
    cfg.update(extra)
    return cfg


def digest(state):
    h = hashlib.sha256()
    for key, value in state.items():
        h.update(key.encode())
        h.update(value.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class Recorder:
    """Hooks one Trainer: _log payloads, and the reads by phase and batch"""

    def __init__(self):
        self.logs, self.reads, self.current = [], {}, None

    def attach(self, trainer):
        trainer._log = lambda payload: self.logs.append({k: v for k, v in payload.items() if k != "duration"})
        unpack = trainer._unpack

        def begin_batch(batch):
            if self.current is not None:
                self.current.append([])
            return unpack(batch)
        trainer._unpack = begin_batch
        for name in ("train", "validate", "evaluate_samples"):
            setattr(trainer, name, self.phased(name, getattr(trainer, name)))
        return trainer

    def phased(self, name, method):
        def call(*a):
            key = " ".join([f"{len(self.reads):02d}", name] + [f"e{v}" for v in a])
            outer, self.current = self.current, self.reads.setdefault(key, [["before the first batch"]])
            try:
                return method(*a)
            finally:
                self.current = outer
        return call

    def read(self, name):
        if self.current is not None:
            self.current[-1].append(name)


@contextlib.contextmanager
def spying(recorder):
    """torch.Tensor's host reads report to the recorder while this is open (device tensors only)"""
    real = {name: getattr(torch.Tensor, name) for name in READS}

    def spy_of(name):
        def spy(self, *a, **k):
            if self.is_cuda:
                recorder.read(name)
            return real[name](self, *a, **k)
        return spy
    for name in READS:
        setattr(torch.Tensor, name, spy_of(name))
    try:
        yield
    finally:
        for name in READS:
            setattr(torch.Tensor, name, real[name])


def scenario(name, drive, seed, six=False, **extra):
    """drive(make) -> {returns}; make(**more) builds a recorded Trainer of this scenario's config"""
    with tempfile.TemporaryDirectory() as tmp:
        home, recorder, text, made = os.getcwd(), Recorder(), io.StringIO(), []

        def make(**more):
            cfg = config(tmp, **extra, **more)
            made.append(recorder.attach(Trainer(cfg, NeuroEncoder(cfg), Volumes(24, 1, six), Volumes(8, 2, six))))
            return made[-1]
        os.chdir(tmp)
        try:
            torch.manual_seed(seed)
            with contextlib.redirect_stdout(text), spying(recorder):
                returns = drive(make)
            files = sorted(STAMP.sub("<stamp>", os.path.relpath(os.path.join(d, f), tmp)) for d, _, fs in os.walk(tmp) for f in fs)
        finally:
            os.chdir(home)
    last = made[-1]
    out = {"stdout": DURATION.sub("", STAMP.sub("<stamp>", text.getvalue())).replace(tmp, "<tmp>").splitlines(), "logs": recorder.logs,
           "reads": recorder.reads, "files": files, "state_dict": digest(last.model.state_dict()), "returns": returns,
           "global_step": last.global_step, "optimizer_steps": last.step.optimizer.steps}
    if last.step.ema is not None:
        out["state_dict_ema"] = digest(last.step.ema.module.state_dict())
    return out


def run_then_validate(make):
    t = make()
    t.run()
    return {"validate": t.validate(2), "evaluate_samples": t.evaluate_samples(), "knn_validate": t.knn_validate(), "linear_validate": t.linear_validate()}


def pretrain(make):
    t = make()
    t.run()
    return {"validate": t.validate(1), "knn_validate": t.knn_validate(), "linear_validate": t.linear_validate(),
            "recon_head": digest(t.step.head.state_dict())}


def save_and_resume(make):
    first = make(TRAINING_SAVE_STATE=True)
    first.epochs = 1                                  # the first of the two epochs the schedule was laid out for
    first.run()
    second = make(TRAINING_SAVE_STATE=True, TRAINING_RESUME_FROM="./results/last_state.pth")
    start = second.start_epoch
    second.run()
    return {"start_epoch": start, "validate": second.validate(2)}


MIM = dict(TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.5, TRAINING_LR_SCHEDULE="cosine", TRAINING_WARMUP_STEPS=2, PRETRAIN_KNN_EVERY=1,
           PRETRAIN_KNN_K=[1, 3], PRETRAIN_LINEAR_EVERY=1, PRETRAIN_LINEAR_L2=[1e-3, 0.1])
SCENARIOS = {
    "a supervised, 7-tuples: dropout, accumulation, weight average, clipping, Mixup":
        (run_then_validate, 11, dict(TRAINING_DROPOUT=0.1, USE_ACCUMULATION=True, TRAINING_ACCUMULATION_STEP=2, TRAINING_EMA_DECAY=0.9,
                                     TRAINING_GRAD_CLIP=1.0, AUGMENT_MIXUP_ALPHA=0.4)),
    "b supervised, 6-tuples, plain": (run_then_validate, 12, dict(six=True)),
    "c regression: huber, weight average, Mixup":
        (run_then_validate, 13, dict(TRAINING_OBJECTIVE="regression", REGRESSION_TARGET_MEAN=[70.0], REGRESSION_TARGET_STD=[8.0], REGRESSION_LOSS="huber",
                                     REGRESSION_HUBER_DELTA=1.5, TRAINING_EMA_DECAY=0.9, AUGMENT_MIXUP_ALPHA=0.4)),
    "d mim: cosine schedule, both probes every epoch": (pretrain, 14, MIM),
    "d2 mim: the probes on two poolings": (pretrain, 15, dict(MIM, PRETRAIN_LINEAR_POOL="mean")),
    "e save the state for one epoch, resume for the next": (save_and_resume, 16, dict(TRAINING_EMA_DECAY=0.9, TRAINING_LR_SCHEDULE="cosine")),
}

only = None if args.only is None else set(args.only.split(","))
result = {name: scenario(name, drive, seed, **extra) for name, (drive, seed, extra) in SCENARIOS.items() if only is None or name.split()[0] in only}
with open(OUT, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(result)} scenarios -> {OUT}")
