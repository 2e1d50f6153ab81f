"""A float64 CPU restatement of the classification metrics (neurovit_amd/csrc/cls_metrics.hip: nv_cls_metrics_update, nv_cls_auc,
nv_segment_labels, nv_cls_metrics_finish) and of ops.ClassificationMetrics.compute(), in numpy.  What it is worth is proven against
scikit-learn / scipy and plain loops in tests/test_cls_metrics_cpu.py; the GPU tests (tests/test_cls_metrics_gpu.py) hold the kernels to it.

It also ASSERTS the conditions its inputs must meet for an exact comparison (check_inputs): every confidence at least 1e-9 / bins away from
a bin edge, and every arg-max either an exact tie of fp32 scores (the lowest index wins) or decided by the fp32 scores themselves.

Measured on the CPU: 3 * randn logits over 4096 rows, C in {2, 3, 5}, 15 bins come no closer to an inner edge than 7.9e-6 of a bin and have
no accidental tie (the top edge, conf = 1, is none: min(bins - 1, .) gives the last bin on both sides of it)."""
import numpy as np

HEAD_NAMES = ("n", "skipped", "nll_sum", "batch_mean_sum", "batches", "brier_sum")
SCALARS = ("n", "skipped", "accuracy", "balanced_accuracy", "macro_f1", "nll", "val_loss", "brier", "ece", "macro_auc")
CLASS_COLS = ("support", "recall", "precision", "f1", "auc")
EDGE_MARGIN = 1e-9          # in units of a bin
SUM_GATE = 1e-9             # double sums and finished metrics of order 1: at most ~1e3 * C terms with a few ulp (2.2e-16) each
FP32_GATE = 1.2e-7          # one fp32 ulp, relative: the finish table is fp32


# ------------------------------------------------------------------ inputs
def logits_case(B, C, seed, scale=3.0):
    """(logits fp32 [B, C], labels int32 [B]) - plain random rows"""
    rng = np.random.default_rng(seed)
    return (scale * rng.standard_normal((B, C))).astype(np.float32), rng.integers(0, C, size=B).astype(np.int32)


def plant(logits, labels, C):
    """Plants the special rows the kernels must get right where B allows (returns the row lists): an exact tie of the two top scores, logits of
    +-80, labels -1 and C, a NaN and an inf logit."""
    B = logits.shape[0]
    rows = {"tie": [], "skipped": [], "big": []}
    if B >= 7:
        logits[1, :] = -1.0
        logits[1, C - 2:] = 2.5                           # the two LAST classes tie: the lower index must win
        rows["tie"].append(1)
        logits[2, :] = -80.0
        logits[2, 0] = 80.0
        rows["big"].append(2)
        labels[3], labels[4] = -1, C
        logits[5, C - 1] = np.nan
        logits[6, 0] = np.inf
        rows["skipped"] += [3, 4, 5, 6]
    return rows


def softmax64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def valid_rows(scores, labels, C):
    return (labels >= 0) & (labels < C) & np.isfinite(scores).all(axis=1)


def probabilities(scores, kind):
    """float64 [B, C] of the valid rows' probabilities under `kind` (invalid rows: whatever comes out, never used)"""
    if kind == "probs":
        return scores.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        z = scores.astype(np.float64)
        m = np.max(scores, axis=1, keepdims=True).astype(np.float64)
        e = np.exp(z - m)
        S = np.zeros(len(z))
        for c in range(z.shape[1]):                        # ascending c, as the kernel
            S = S + e[:, c]
        return e / S[:, None]


def check_inputs(scores, labels, C, bins, kind):
    """Asserts the edge margin of every valid row's confidence and returns the rows whose two top fp32 scores tie exactly."""
    ok = valid_rows(scores, labels, C)
    p = probabilities(scores, kind)
    ties = []
    for b in np.nonzero(ok)[0]:
        top = np.sort(scores[b])[::-1]
        if top[0] == top[1]:
            ties.append(int(b))
        conf = p[b, int(np.argmax(scores[b]))] * bins
        if conf >= bins - EDGE_MARGIN:                     # at or beside the top edge: min(bins - 1, .) gives the last bin on both sides
            continue
        assert abs(conf - np.round(conf)) >= EDGE_MARGIN, f"row {b}: confidence {conf / bins!r} lies on a bin edge"
    return ties


# ------------------------------------------------------------------ nv_cls_metrics_update
def new_state(C, bins):
    s = {k: 0.0 for k in HEAD_NAMES}
    s.update(confusion=np.zeros((C, C), np.int64), bin_count=np.zeros(bins, np.int64), bin_conf=np.zeros(bins), bin_correct=np.zeros(bins, np.int64))
    return s


def update_ref(state, scores, labels, C, bins, kind="logits", argmax_ge=False):
    """One call of nv_cls_metrics_update on `state` (in place).  Returns (bank probabilities fp32 [B, C], bank labels int32 [B]).
    argmax_ge: the planted defect - the LAST index of the maximum instead of the first."""
    B = scores.shape[0]
    ok = valid_rows(scores, labels, C)
    p = probabilities(scores, kind)
    bank, bank_labels = np.zeros((B, C), np.float32), np.full(B, -1, np.int32)
    nll_sum, n = 0.0, 0
    for b in range(B):
        if not ok[b]:
            state["skipped"] += 1
            continue
        y, z = int(labels[b]), scores[b]
        pred = int(C - 1 - np.argmax(z[::-1])) if argmax_ge else int(np.argmax(z))      # np.argmax: the first index of the maximum
        if kind == "logits":
            z64, m = z.astype(np.float64), np.float64(z.max())
            S = 0.0
            for c in range(C):
                S += np.exp(z64[c] - m)
            nll = (m + np.log(S)) - z64[y]
        else:
            with np.errstate(divide="ignore"):
                nll = -np.log(p[b, y])
        brier = float(((p[b] - np.eye(C)[y]) ** 2).sum())
        conf = p[b, pred]
        k = min(bins - 1, max(0, int(conf * bins)))
        state["confusion"][y, pred] += 1
        state["bin_count"][k] += 1
        state["bin_conf"][k] += conf
        state["bin_correct"][k] += pred == y
        state["brier_sum"] += brier
        nll_sum += nll
        n += 1
        bank[b], bank_labels[b] = p[b].astype(np.float32), y
    state["n"] += n
    state["nll_sum"] += nll_sum
    if n:
        state["batch_mean_sum"] += nll_sum / n
        state["batches"] += 1
    return bank, bank_labels


# ------------------------------------------------------------------ nv_cls_auc
def auc_ref(probs, labels, C, half=True):
    """float64 [C, 5]: auc, n_pos, n_neg, gt, eq by counting pairs on the fp32 values.  half=False: the planted defect, ties not counted."""
    out = np.full((C, 5), np.nan)
    usable = (labels >= 0) & (labels < C)
    for c in range(C):
        pos, neg = probs[usable & (labels == c), c], probs[usable & (labels != c), c]
        gt = int((pos[:, None] > neg[None, :]).sum())
        eq = int((pos[:, None] == neg[None, :]).sum())
        n_pos, n_neg = len(pos), len(neg)
        if n_pos and n_neg:
            out[c, 0] = (float(gt) + (0.5 * float(eq) if half else 0.0)) / (float(n_pos) * float(n_neg))
        out[c, 1:] = n_pos, n_neg, gt, eq
    return out


# ------------------------------------------------------------------ segments
def segment_mean_ref(src, groups, G):
    """fp32 [G, w]: per segment the double sum of the fp32 rows in ascending row order, divided in double, rounded once; empty: zeros"""
    out = np.zeros((G, src.shape[1]), np.float32)
    for g in range(G):
        rows = np.nonzero(groups == g)[0]
        if len(rows):
            s = np.zeros(src.shape[1])
            for r in rows:
                s = s + src[r].astype(np.float64)
            out[g] = (s / float(len(rows))).astype(np.float32)
    return out


def segment_labels_ref(labels, groups, G):
    """(int32 [G] label of each segment's first row, -1 for an empty segment; the number of segments that hold another label >= 0)"""
    out, mixed = np.full(G, -1, np.int32), 0
    for g in range(G):
        rows = np.nonzero(groups == g)[0]
        if len(rows):
            out[g] = labels[rows[0]]
            mixed += int(any(labels[r] >= 0 and labels[r] != out[g] for r in rows[1:]))
    return out, mixed


# ------------------------------------------------------------------ nv_cls_metrics_finish
def _nanmean(values, zero_for_nan=False):
    v = np.asarray(values, np.float64)
    if zero_for_nan:                                       # the planted defect: an empty class counts as 0
        return float(np.where(np.isnan(v), 0.0, v).mean())
    keep = v[~np.isnan(v)]
    return float(keep.sum() / len(keep)) if len(keep) else float("nan")


def finish_ref(state, C, bins, auc=None, macro_zero=False, row_mean_loss=False):
    """{scalar names: float, "class": float64 [C, 5], "confusion": int64 [C, C]} in double; undefined = NaN"""
    cm, n, nan = state["confusion"].astype(np.float64), float(state["n"]), float("nan")
    support, predicted, tp = cm.sum(axis=1), cm.sum(axis=0), np.diag(cm)
    with np.errstate(invalid="ignore", divide="ignore"):
        recall = np.where(support > 0, tp / support, nan)
        precision = np.where(predicted > 0, tp / predicted, nan)
        f1 = np.where(support + predicted > 0, 2 * tp / (support + predicted), nan)
    a = np.full(C, nan) if auc is None else np.asarray(auc, np.float64)[:, 0]
    got = {"n": n, "skipped": float(state["skipped"]), "class": np.stack([support, recall, precision, f1, a], axis=1), "confusion": state["confusion"].copy()}
    any_row = n > 0
    got["accuracy"] = tp.sum() / n if any_row else nan
    got["balanced_accuracy"] = _nanmean(recall, macro_zero) if any_row else nan
    got["macro_f1"] = _nanmean(f1, macro_zero) if any_row else nan
    got["nll"] = state["nll_sum"] / n if any_row else nan
    got["val_loss"] = (got["nll"] if row_mean_loss else state["batch_mean_sum"] / state["batches"]) if state["batches"] > 0 else nan
    got["brier"] = state["brier_sum"] / n if any_row else nan
    got["ece"] = float(np.abs(state["bin_correct"] - state["bin_conf"]).sum()) / n if any_row else nan
    got["macro_auc"] = _nanmean(a, macro_zero)
    return got


def table_ref(fin, C):
    """the fp64 values of nv_cls_metrics_finish's table in its order: scalars, [C, 5], [C, C]"""
    return np.concatenate([[fin[k] for k in SCALARS], fin["class"].reshape(-1), fin["confusion"].astype(np.float64).reshape(-1)])


# ------------------------------------------------------------------ ops.ClassificationMetrics.compute()
def compute_ref(batches, C, bins=15, kind="logits", capacity=True, groups=None, bank=None):
    """batches: [(scores, labels)].  groups: host ids per row of the concatenated batches (or None).  bank: (probs fp32, labels) to pool and
    rank INSTEAD of the restated bank (the device's own, once it was held to the restated one within an ulp: the pooled means then carry the
    same bits on both sides).  Returns (volume finish dict, subject finish dict or None, extras)."""
    state = new_state(C, bins)
    banks = [update_ref(state, s, l, C, bins, kind) for s, l in batches]
    probs, labels = np.concatenate([b[0] for b in banks]), np.concatenate([b[1] for b in banks])
    extras = {"state": state, "bank": probs, "bank_labels": labels}
    if bank is not None:
        probs, labels = bank
    auc = auc_ref(probs, labels, C) if capacity else None
    extras["auc"] = auc
    fin, sub = finish_ref(state, C, bins, auc), None
    if capacity and groups is not None and groups.max() >= 0:
        G = int(groups.max()) + 1
        pooled = segment_mean_ref(probs, groups, G)
        sl, mixed = segment_labels_ref(labels, groups, G)
        check_inputs(pooled, sl, C, bins, "probs")
        sstate = new_state(C, bins)
        update_ref(sstate, pooled, sl, C, bins, "probs")
        sauc = auc_ref(pooled, sl, C)
        sub = finish_ref(sstate, C, bins, sauc)
        extras.update(subject_state=sstate, subject_probs=pooled, subject_labels=sl, subject_mixed=mixed, subject_auc=sauc)
    return fin, sub, extras
