"""Frozen-feature evaluation of the encoder: a bank of embeddings, the weighted k-nearest-neighbour probe (DINO's classifier) over it,
subject-level pooling (csrc/features.hip: ops.pool_features / knn_topk / knn_vote; csrc/segments.hip: ops.Segments) and the linear probe (LinearProbe /
linear_evaluate at the end of this file; csrc/probe.hip).

    bank = FeatureBank(dim, capacity=len(train_set)).fill(model, train_loader)
    out = knn_evaluate(bank, val_features, labels=val_labels, k=(5, 10, 20), query_groups=val_subjects)

The similarity is the plain dot product of the stored rows: extract with normalize=True (the default here) for cosine similarity.  The volumes
of one subject are near-duplicates: give the bank its rows' subjects (`groups`) and the queries theirs (`query_groups`, the same ids) and no
query is answered by its own subject; scores are also reported per subject.  PyTorch owns the buffers; every FLOP of extraction, search, vote
and pooling runs in libneurovit_hip.so.  There is no CPU fallback."""
from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Tuple, Union

import torch

from . import ops


def _extract(model, x, **kw) -> torch.Tensor:
    """model.extract_features (NeuroEncoder: x [B, H, W, D]) or model.forward_features (ViT: x [B, C, F, H, W])"""
    fn = getattr(model, "extract_features", None) or getattr(model, "forward_features", None)
    if fn is None:
        raise TypeError(f"{type(model).__name__} has neither extract_features nor forward_features")
    return fn(x, **kw)


class GroupIndex:
    """Subjects (any hashable: the strings a dataset yields, ints) -> dense integer ids, shared by a bank and its queries."""

    def __init__(self):
        self.ids: Dict[object, int] = {}

    def __call__(self, subjects) -> torch.Tensor:
        if torch.is_tensor(subjects):
            subjects = subjects.reshape(-1).tolist()
        return torch.tensor([self.ids.setdefault(s, len(self.ids)) for s in subjects], dtype=torch.int32)

    def __len__(self):
        return len(self.ids)


class FeatureBank:
    """Preallocated device bank: `features` fp32 [capacity, dim], `labels` int32 [capacity] (-1 = none), `targets` fp32 [capacity, K] (NaN =
    missing; allocated by num_targets) and `groups` int32 [capacity] (-1 = none), of which the first `size` rows are filled.  append() writes
    the model's features straight into their rows (no cat); the host copy of the groups is kept for by_group()."""

    def __init__(self, dim: int, capacity: int, device="cuda", num_targets: int = 0):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("FeatureBank lives on the MI355X (cuda) device - there is no CPU fallback")
        if dim < 4 or dim % 4 or capacity < 1:
            raise ValueError(f"FeatureBank: dim = {dim} must be a positive multiple of 4 (nv_knn_topk), capacity = {capacity} at least 1")
        self.dim, self.capacity, self.size = int(dim), int(capacity), 0
        self.features = torch.zeros((capacity, dim), dtype=torch.float32, device=self.device)
        self.labels = torch.full((capacity,), -1, dtype=torch.int32, device=self.device)
        self.targets = torch.full((capacity, num_targets), float("nan"), dtype=torch.float32, device=self.device) if num_targets else None
        self.groups = torch.full((capacity,), -1, dtype=torch.int32, device=self.device)
        self._host_groups = torch.full((capacity,), -1, dtype=torch.int32)
        self.has_groups = False
        self.has_labels = False               # any label was given (what a classification LinearProbe asks for)

    @classmethod
    def from_features(cls, features: torch.Tensor, labels=None, targets=None, groups=None) -> "FeatureBank":
        """a full bank around features fp32 [N, dim] that exist already (copied)"""
        N, dim = features.shape
        bank = cls(dim, N, features.device, num_targets=0 if targets is None else targets.shape[1])
        bank.features.copy_(features)
        bank._annotate(0, N, labels, groups, targets)
        bank.size = N
        return bank

    def _annotate(self, row0: int, B: int, labels, groups, targets) -> None:
        if labels is not None:
            self.labels[row0:row0 + B] = torch.as_tensor(labels).reshape(-1).to(self.device, torch.int32)
            self.has_labels = True
        if targets is not None:
            if self.targets is None:
                raise ValueError("FeatureBank: built without targets - pass num_targets")
            self.targets[row0:row0 + B] = torch.as_tensor(targets, dtype=torch.float32).reshape(B, -1).to(self.device)
        if groups is not None:
            g = ops.host_ids(groups, B, "FeatureBank groups")
            self._host_groups[row0:row0 + B] = g
            self.groups[row0:row0 + B] = g.to(self.device)
            self.has_groups = True

    def append(self, model, x, labels=None, groups=None, targets=None, pool=None, normalize: bool = True) -> torch.Tensor:
        """The features of the batch x into the next rows (the extraction writes them in place: out / row0); returns those rows."""
        B = x.shape[0]
        if self.size + B > self.capacity:
            raise ValueError(f"FeatureBank: {self.size} + {B} rows exceed the capacity {self.capacity}")
        rows = _extract(model, x, pool=pool, normalize=normalize, out=self.features, row0=self.size)
        self._annotate(self.size, B, labels, groups, targets)
        self.size += B
        return rows

    def fill(self, model, loader, unpack: Optional[Callable] = None, transform: Optional[Callable] = None, pool=None, normalize: bool = True,
             group_index: Optional[GroupIndex] = None) -> "FeatureBank":
        """append() over a loader.  unpack(batch) -> (x, labels or None, subjects or None, targets or None); the default reads the dataset's
        batches (subject first, volume third, label last).  transform: applied to x on the device (the Trainer's centre window).
        group_index: maps the subjects to ids (shared with the queries); without one, integer subjects are taken as they are."""
        unpack = unpack or (lambda b: (b[2], b[-1], b[0], None))
        for batch in loader:
            x, labels, subjects, targets = unpack(batch)
            x = x.to(self.device)
            if transform is not None:
                x = transform(x)
            groups = None if subjects is None else (group_index(subjects) if group_index is not None else subjects)
            self.append(model, x, labels, groups, targets, pool=pool, normalize=normalize)
        return self

    def view(self) -> torch.Tensor:
        return self.features[:self.size]

    def by_group(self, normalize: bool = True) -> "FeatureBank":
        """The subject-level bank: one row per group id 0 .. G - 1 = the mean of its rows' features (nv_segment_mean; re-normalised by default,
        a group without rows stays zero), the label / targets of its first row, groups = arange."""
        if not self.has_groups or self.size == 0:
            raise ValueError("FeatureBank.by_group: the bank has no groups")
        subjects = ops.Segments(self._host_groups[:self.size])
        G = subjects.G
        out = FeatureBank(self.dim, G, self.device, num_targets=0 if self.targets is None else self.targets.shape[1])
        subjects.mean(self.view(), out=out.features)
        if normalize:
            ops.pool_features(out.features.view(G, 1, self.dim), "cls", True, out=out.features)
        out.labels.copy_(subjects.labels(self.labels[:self.size])[0])
        if self.targets is not None:
            first = subjects.order[subjects.offsets[:-1].clamp(max=self.size - 1).long()].long()
            filled = subjects.offsets[1:] > subjects.offsets[:-1]
            out.targets.copy_(torch.where(filled[:, None], self.targets[first], torch.full_like(self.targets[first], float("nan"))))
        out._annotate(0, G, None, torch.arange(G, dtype=torch.int32), None)
        out.has_labels = self.has_labels
        out.size = G
        return out


def _ks(k) -> Tuple[int, ...]:
    ks = (int(k),) if isinstance(k, int) else tuple(int(v) for v in k)
    if not ks or min(ks) < 1 or max(ks) > 128:
        raise ValueError(f"k = {k!r}: one or several values in [1, 128]")
    return ks


def knn_predict(bank: FeatureBank, queries: torch.Tensor, k: Union[int, Sequence[int]] = 20, temperature: float = 0.07, weights: str = "softmax",
                query_groups=None, task: str = "classification", num_classes: Optional[int] = None, splits: int = 0):
    """The weighted kNN prediction of queries fp32 [Nq, dim] against the bank: one nv_knn_topk pass at max(k), one nv_knn_vote per k.
    Returns (predictions, scores, idx, sim), device tensors: classification - predictions int32 [Nq] (-1: no usable neighbour), scores fp32
    [Nq, C]; regression - predictions fp32 [Nq, K], scores None; for several k, predictions and scores are dicts {k: tensor}.  idx int32 / sim fp32
    [Nq, max(k)], best first (equal sim to the lower bank row, unfilled slots -1 / -inf).  query_groups (ids as the bank's groups): a bank row of
    the query's own group is never a neighbour.  num_classes: default the bank's largest label + 1 (one host read - pass it to avoid that)."""
    if task not in ("classification", "regression"):
        raise ValueError(f"knn_predict: task must be 'classification' or 'regression', got {task!r}")
    if bank.size < 1:
        raise ValueError("knn_predict: the bank is empty")
    ks = _ks(k)
    qg = bg = None
    if query_groups is not None:
        if not bank.has_groups:
            raise ValueError("knn_predict: query_groups given, but the bank has no groups")
        qg = ops.host_ids(query_groups, queries.shape[0], "query_groups").to(queries.device)
        bg = bank.groups[:bank.size]
    idx, sim = ops.knn_topk(queries, bank.view(), max(ks), qg, bg, splits=splits)
    preds, scores = {}, {}
    for kk in ks:
        if task == "classification":
            C = int(num_classes) if num_classes is not None else int(bank.labels[:bank.size].max().item()) + 1
            scores[kk], preds[kk] = ops.knn_vote(idx, sim, kk, labels=bank.labels[:bank.size], num_classes=C, weights=weights, temperature=temperature)
        else:
            if bank.targets is None:
                raise ValueError("knn_predict: a regression vote needs a bank with targets")
            preds[kk], scores[kk] = ops.knn_vote(idx, sim, kk, targets=bank.targets[:bank.size], weights=weights, temperature=temperature), None
    if isinstance(k, int):
        return preds[ks[0]], scores[ks[0]], idx, sim
    return preds, (scores if task == "classification" else None), idx, sim


def knn_evaluate(bank: FeatureBank, queries: torch.Tensor, labels=None, targets=None, k: Union[int, Sequence[int]] = 20, temperature: float = 0.07,
                 weights: str = "softmax", query_groups=None, num_classes: Optional[int] = None, splits: int = 0) -> dict:
    """knn_predict plus its score against the truth; one host read at the end.  labels int [Nq] -> {"acc": {k: float}} per volume and, with
    query_groups, {"subject_acc": {k: float}}: the volumes' scores averaged per subject (nv_segment_mean), arg-max, against the label of the
    subject's first volume.  targets fp32 [Nq, K] (NaN = missing) -> {"mae": {k: [K floats]}} through ops.RegressionMetrics (raw scale), and
    "subject_mae" likewise on the per-subject means of predictions and targets.  Also returns the device tensors under "predictions", "scores",
    "idx", "sim" (of every k)."""
    if (labels is None) == (targets is None):
        raise ValueError("knn_evaluate: give labels (classification) or targets (regression), one of the two")
    ks = _ks(k)
    task = "classification" if labels is not None else "regression"
    preds, scores, idx, sim = knn_predict(bank, queries, ks, temperature, weights, query_groups, task, num_classes, splits)
    subjects = None if query_groups is None else ops.Segments(ops.host_ids(query_groups, queries.shape[0], "query_groups"))
    variants = [(kk, preds[kk], scores[kk] if scores is not None else None) for kk in ks]

    def voted(pooled):                                           # a subject without a positive vote has no class: -1, a miss
        best, cls = pooled.max(dim=1)
        return torch.where(best > 0, cls.to(torch.int32), torch.full_like(cls, -1, dtype=torch.int32))
    return {"predictions": preds, "scores": scores, "idx": idx, "sim": sim,
            **_score(variants, queries, subjects, labels, targets, None if bank.targets is None else bank.targets.shape[1], voted)}


def _score(variants, queries, subjects, labels, targets, K, subject_class) -> dict:
    """The score of [(key, predictions, scores or None)] against labels int [Nq] -> {"acc": {key: float}} or targets fp32 [Nq, K] -> {"mae":
    {key: [K floats]}} (ops.RegressionMetrics, raw scale); with the ops.Segments of the queries' subjects also "subject_acc" - the
    scores averaged per subject (nv_segment_mean), subject_class of them, against the label of the subject's first volume - or
    "subject_mae" on the NaN-aware per-subject means of predictions and targets.  Device expressions throughout, ONE host read."""
    keys, (Nq, dev) = [key for key, _, _ in variants], (queries.shape[0], queries.device)
    if labels is not None:
        y = torch.as_tensor(labels).reshape(-1).to(dev, torch.int32)
        cells = [(pred == y).float().mean() for _, pred, _ in variants]
        if subjects is not None:
            filled = subjects.offsets[1:] > subjects.offsets[:-1]       # (an empty subject's label is -1, and so is the class of its zero votes)
            y_subject = subjects.labels(y)[0]
            for _, _, score in variants:
                cls = subject_class(subjects.mean(score))
                cells.append(((cls == y_subject) & filled).float().sum() / filled.float().sum().clamp(min=1))
        host = torch.stack(cells).cpu().tolist()                 # the one host read
        names = ("acc", "subject_acc")
    else:
        t = ops.reg_targets(targets, Nq, K).to(dev)

        def table(pred, truth):
            m = ops.RegressionMetrics(t.shape[1], device=dev)
            m.update(pred, truth)
            return m.compute_device()
        tables = [table(pred, t) for _, pred, _ in variants]
        if subjects is not None:
            t_subject = subjects.nanmean(t)
            tables += [table(subjects.nanmean(pred), t_subject) for _, pred, _ in variants]
        host = torch.stack(tables).cpu()[:, :, 1].tolist()       # the one host read; column 1: the mean absolute error
        names = ("mae", "subject_mae")
    out = {names[0]: dict(zip(keys, host[:len(keys)]))}
    if subjects is not None:
        out[names[1]] = dict(zip(keys, host[len(keys):]))
    return out


# ---------------------------------------------------------------------------------------------------- the linear probe
def _l2s(l2) -> Tuple[float, ...]:
    vals = (float(l2),) if isinstance(l2, (int, float)) and not isinstance(l2, bool) else tuple(float(v) for v in l2)
    if not vals or any(not (v >= 0.0) or v == float("inf") for v in vals):
        raise ValueError(f"LinearProbe: l2 = {l2!r}: one or several finite values >= 0 (the coupled L2 strength of each head)")
    return vals


class LinearProbe:
    """H linear read-outs of frozen features, one per L2 strength, trained side by side over ONE read of the bank per step (DINOv2's grid of
    probes), on the native kernels of csrc/probe.hip (ops.probe_stats / probe_grad / probe_step / probe_predict).  Head h minimises
    J_h = L_h + (l2_h / 2) |W_h|^2 (bias not penalised, the L2 term COUPLED - inside the gradient, not AdamW's decay) with full-batch Adam:
    softmax cross-entropy over the bank's labels (rows labelled outside [0, C) carry no loss) or, with num_targets, the squared error on the
    standardised targets (NaN = missing, every target column with its own count of observed cells).

        probe = LinearProbe(bank.dim, num_classes=2).fit(bank)            # .history: the loss per step and head, a device tensor
        out = linear_evaluate(probe, val_features, labels=val_labels, query_groups=val_subjects)

    weight [H, C, dim] and bias [H, C] are views of the [H C, dim] / [H C] arrays the kernels step.  There is no sampling and no seed: a fit
    is a pure function of the bank, bit for bit.  No CPU fallback."""

    def __init__(self, dim: int, num_classes: Optional[int] = None, num_targets: Optional[int] = None, l2=(1e-4, 1e-3, 1e-2, 1e-1), device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LinearProbe lives on the MI355X (cuda) device - there is no CPU fallback")
        if (num_classes is None) == (num_targets is None):
            raise ValueError("LinearProbe: give num_classes (classification) or num_targets (regression), one of the two")
        if int(dim) < 4 or int(dim) % 4 or int(dim) > 1024:
            raise ValueError(f"LinearProbe: dim = {dim} must be a multiple of 4 up to 1024 (nv_probe_grad)")
        self.task = "classification" if num_classes is not None else "regression"
        self.dim, self.C = int(dim), int(num_classes if num_classes is not None else num_targets)
        if self.C < 1 or self.C > 32 or (self.task == "classification" and self.C < 2):
            raise ValueError(f"LinearProbe: C = {self.C} columns per head: 2 .. 32 classes or 1 .. 32 targets (one nv_probe_grad pass holds 32 columns)")
        self.l2 = _l2s(l2)
        self.H = len(self.l2)
        self._W = torch.zeros((self.H * self.C, self.dim), device=self.device)
        self._b = torch.zeros(self.H * self.C, device=self.device)
        self.weight, self.bias = self._W.view(self.H, self.C, self.dim), self._b.view(self.H, self.C)
        self.mean = self.rstd = self.target_mean = self.target_std = None
        self.history: Optional[torch.Tensor] = None

    def _passes(self):
        """head ranges of at most 32 columns each: one nv_probe_grad call per range and step"""
        per = 32 // self.C
        return [(h, min(h + per, self.H)) for h in range(0, self.H, per)]

    def fit(self, bank: FeatureBank, steps: int = 500, lr: float = 0.01, schedule: str = "cosine", standardize: bool = True, class_weight=None,
            task: Optional[str] = None, target_mean=None, target_std=None, betas=(0.9, 0.999), eps: float = 1e-8, max_blocks: int = 0) -> "LinearProbe":
        """Full-batch Adam over bank.view() from zero weights: `steps` steps at lr_at(k) of LRSchedule(lr, steps, kind=schedule) (cosine to 0).
        standardize: z = (x - mean) rstd with the bank's own column statistics (kept for predict).  class_weight: fp32 [C], classification only.
        target_mean / target_std: [K] (default: the statistics of the bank's observed targets; a constant target column gets std 1).  Three
        launches per step and pass, no host read; self.history: fp32 [steps, H] on the device."""
        from .optim import LRSchedule
        task = self.task if task is None else task
        if task not in ("classification", "regression"):
            raise ValueError(f"LinearProbe.fit: task must be 'classification' or 'regression', got {task!r}")
        if task != self.task:
            raise ValueError(f"LinearProbe.fit: this probe was built for {self.task} (num_classes / num_targets), not {task}")
        if bank.size < 1:
            raise ValueError("LinearProbe.fit: the bank is empty")
        if bank.dim != self.dim:
            raise ValueError(f"LinearProbe.fit: the bank's features have {bank.dim} columns, the probe {self.dim}")
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"LinearProbe.fit: steps = {steps!r} must be an integer >= 1")
        N, X, C = bank.size, bank.view(), self.C
        sched = LRSchedule(lr, steps, kind=schedule)
        labels = targets = cw = None
        if task == "classification":
            if not bank.has_labels:
                raise ValueError("LinearProbe.fit: a classification probe needs a bank with labels, this one was given none")
            labels = bank.labels[:N]
            if class_weight is not None:
                cw = torch.as_tensor(class_weight, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
                if cw.numel() != C:
                    raise ValueError(f"LinearProbe.fit: class_weight has {cw.numel()} entries for {C} classes")
            denom = ops.probe_stats(labels=labels, num_classes=C, class_weight=cw)["denom"]
        else:
            if class_weight is not None:
                raise ValueError("LinearProbe.fit: class_weight belongs to classification, not to regression")
            if bank.targets is None or bank.targets.shape[1] != C:
                raise ValueError(f"LinearProbe.fit: a regression probe of {C} targets needs a bank with targets [*, {C}]")
            targets = bank.targets[:N]
            st = ops.probe_stats(targets, skip_nan=True, eps=0.0)
            denom = st["count"]
            vec = lambda t: torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            self.target_mean = st["mean"] if target_mean is None else vec(target_mean)
            self.target_std = torch.where(st["std"] > 0, st["std"], torch.ones_like(st["std"])) if target_std is None else vec(target_std)
            if self.target_mean.numel() != C or self.target_std.numel() != C:
                raise ValueError(f"LinearProbe.fit: target_mean / target_std must have {C} entries")
        self.mean = self.rstd = None
        if standardize:
            st = ops.probe_stats(X)
            self.mean, self.rstd = st["mean"], st["rstd"]
        self._W.zero_()
        self._b.zero_()
        self.history = torch.empty((steps, self.H), device=self.device)
        for h0, h1 in self._passes():
            rows = slice(h0 * C, h1 * C)
            W, b = self._W[rows], self._b[rows]
            dW, db = torch.empty_like(W), torch.empty_like(b)
            mW, vW, mb, vb = torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(b)
            ws = torch.empty(ops.probe_grad_workspace_bytes(N, self.dim, W.shape[0]), dtype=torch.uint8, device=self.device)
            for k in range(1, steps + 1):
                sizes, _ = ops.probe_adam_constants(k, [sched.lr_at(k)] * (h1 - h0), betas)
                heads = ops.probe_heads(h1 - h0, C, self.l2[h0:h1], sizes)
                ops.probe_grad(X, W, b, heads, denom, labels=labels, targets=targets, mean=self.mean, rstd=self.rstd, class_weight=cw,
                               target_mean=self.target_mean if targets is not None else None, target_std=self.target_std if targets is not None else None,
                               max_blocks=max_blocks, out=(dW, db, self.history[k - 1, h0:h1]), workspace=ws)
                ops.probe_step(W, b, dW, db, mW, vW, mb, vb, heads, k, betas, eps)
        return self

    def logits(self, queries: torch.Tensor, want_probs: bool = False):
        """(logits fp32 [Nq, H C], probs or None): one nv_probe_predict per pass, written into its column window"""
        Nq = queries.shape[0]
        logits = torch.empty((Nq, self.H * self.C), device=self.device)
        probs = torch.empty_like(logits) if want_probs else None
        for h0, h1 in self._passes():
            rows = slice(h0 * self.C, h1 * self.C)
            ops.probe_predict(queries, self._W[rows], self._b[rows], h1 - h0, self.C, mean=self.mean, rstd=self.rstd, logits=logits[:, rows],
                              probs=None if probs is None else probs[:, rows])
        return logits, probs

    def predict(self, queries: torch.Tensor, head: Optional[int] = None):
        """Classification: (pred int32 [H, Nq], probs fp32 [H, Nq, C]) - the fp32 softmax over each head's own columns, arg-max with ties to
        the lower class; regression: predictions on the RAW scale fp32 [H, Nq, K].  head = h: that head alone ([Nq], [Nq, C] / [Nq, K])."""
        if head is not None and not 0 <= int(head) < self.H:
            raise ValueError(f"LinearProbe.predict: head = {head} outside [0, {self.H})")
        Nq = queries.shape[0]
        logits, probs = self.logits(queries, want_probs=self.task == "classification")
        if self.task == "classification":
            probs = probs.view(Nq, self.H, self.C).permute(1, 0, 2).contiguous()
            pred = probs.argmax(dim=2).to(torch.int32)
            return (pred, probs) if head is None else (pred[head], probs[head])
        raw = logits.view(Nq, self.H, self.C)
        if self.target_std is not None:
            raw = raw * self.target_std + self.target_mean
        raw = raw.permute(1, 0, 2).contiguous()
        return raw if head is None else raw[head]

    def state_dict(self) -> dict:
        out = dict(weight=self.weight.clone(), bias=self.bias.clone(), l2=torch.tensor(self.l2, dtype=torch.float64), task=self.task)
        for name in ("mean", "rstd", "target_mean", "target_std"):
            t = getattr(self, name)
            out[name] = None if t is None else t.clone()
        return out

    def load_state_dict(self, state: dict) -> "LinearProbe":
        if state["task"] != self.task or tuple(state["weight"].shape) != (self.H, self.C, self.dim):
            raise ValueError(f"LinearProbe.load_state_dict: a {state['task']} probe of shape {tuple(state['weight'].shape)} does not fit this "
                             f"{self.task} probe of shape {(self.H, self.C, self.dim)}")
        self.weight.copy_(state["weight"])
        self.bias.copy_(state["bias"])
        self.l2 = tuple(float(v) for v in state["l2"].tolist())
        for name in ("mean", "rstd", "target_mean", "target_std"):
            t = state.get(name)
            setattr(self, name, None if t is None else t.to(self.device, torch.float32).contiguous().clone())
        return self


def linear_evaluate(probe: LinearProbe, queries: torch.Tensor, labels=None, targets=None, query_groups=None) -> dict:
    """LinearProbe.predict plus its score against the truth, per head, keyed by the head's l2; one host read at the end.  labels int [Nq] ->
    {"acc": {l2: float}} per volume and, with query_groups, {"subject_acc": {l2: float}}: the volumes' probabilities averaged per subject
    (nv_segment_mean), arg-max, against the label of the subject's first volume.  targets fp32 [Nq, K] (NaN = missing) -> {"mae": {l2: [K
    floats]}} through ops.RegressionMetrics (raw scale) and "subject_mae" on the per-subject means of predictions and targets.  Also returns
    the device tensors under "predictions" (and "probs")."""
    if (labels is None) == (targets is None):
        raise ValueError("linear_evaluate: give labels (classification) or targets (regression), one of the two")
    if (labels is not None) != (probe.task == "classification"):
        raise ValueError(f"linear_evaluate: a {probe.task} probe, but {'labels' if labels is not None else 'targets'} were given")
    subjects = None if query_groups is None else ops.Segments(ops.host_ids(query_groups, queries.shape[0], "query_groups"))
    if labels is not None:
        pred, probs = probe.predict(queries)
        out = {"predictions": pred, "probs": probs}
        variants = [(l2, pred[h], probs[h]) for h, l2 in enumerate(probe.l2)]
    else:
        raw = probe.predict(queries)
        out = {"predictions": raw}
        variants = [(l2, raw[h], None) for h, l2 in enumerate(probe.l2)]
    return {**out, **_score(variants, queries, subjects, labels, targets, probe.C, lambda pooled: pooled.argmax(dim=1).to(torch.int32))}
