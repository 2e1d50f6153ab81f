"""What the float64 restatement of the classification metrics (tests/cls_metrics_ref.py) is worth: held to scikit-learn, scipy and plain loops,
with planted defects that must change the result on the test inputs; the refusals and the default-path guarantee that can be shown without a
GPU; the host side of cls_metrics.hip under the host sanitizers (a stand-alone program, nothing loaded into Python is sanitised)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cls_metrics_ref as R
import weights as W
from neurovit_amd._cabi import CLS_CLASS_METRIC_NAMES, CLS_METRIC_NAMES      # the restatement restates THESE columns: no binding, no test

assert CLS_METRIC_NAMES == R.SCALARS and CLS_CLASS_METRIC_NAMES == R.CLASS_COLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(257, 2), (257, 3), (300, 5)]
BINS = 15


def planted_case(B, C, seed):
    z, y = R.logits_case(B, C, seed)
    rows = R.plant(z, y, C)
    assert R.check_inputs(z, y, C, BINS, "logits") == rows["tie"]
    return z, y, rows


# ------------------------------------------------------------------ the condition the header of the restatement states
def test_random_logits_keep_the_margins_the_restatement_asserts():
    for C in (2, 3, 5):
        z, y = R.logits_case(4096, C, 7 + C)
        assert R.check_inputs(z, y, C, BINS, "logits") == []                    # no accidental tie
        conf = R.probabilities(z, "logits").max(axis=1) * BINS
        conf = conf[conf < BINS - 0.5]                                           # (the top edge is none: min(bins - 1, .) holds on both sides of it)
        assert np.abs(conf - np.round(conf)).min() > 3e-6                        # measured: 2.4e-5, 7.9e-6, 1.6e-4 of a bin for C = 2, 3, 5
    on_edge = np.array([[0.0, 0.0, 0.0]], np.float32)                            # three-way tie: conf = 1/3 = bin edge 5 of 15
    with pytest.raises(AssertionError):
        R.check_inputs(on_edge, np.array([0], np.int32), 3, BINS, "logits")


# ------------------------------------------------------------------ against independent code
@pytest.mark.parametrize("B,C", SHAPES)
def test_update_and_finish_against_sklearn_and_plain_loops(B, C):
    from sklearn.metrics import balanced_accuracy_score, confusion_matrix, f1_score, log_loss
    z, y, rows = planted_case(B, C, 10 * B + C)
    state = R.new_state(C, BINS)
    bank, bank_labels = R.update_ref(state, z, y, C, BINS)
    fin = R.finish_ref(state, C, BINS)
    ok = R.valid_rows(z, y, C)
    assert fin["n"] == ok.sum() and fin["skipped"] == len(rows["skipped"]) == (~ok).sum()
    p = torch.softmax(torch.from_numpy(z[ok]).double(), dim=1).numpy()
    pred = torch.from_numpy(z[ok]).argmax(dim=1).numpy()
    pred[np.isin(np.nonzero(ok)[0], rows["tie"])] = C - 2                        # the tie rows: the lower of the two tied indices
    yt = y[ok]
    assert np.array_equal(fin["confusion"], confusion_matrix(yt, pred, labels=list(range(C))))
    assert abs(fin["accuracy"] - (pred == yt).mean()) < 1e-15
    assert abs(fin["balanced_accuracy"] - balanced_accuracy_score(yt, pred)) < 1e-12
    assert abs(fin["macro_f1"] - f1_score(yt, pred, average="macro")) < 1e-12
    big = np.isin(np.nonzero(ok)[0], rows["big"])                                # log_loss clips at eps: the +-80 row (nll 160 or 0, exactly) by hand
    by_hand = sum(0.0 if y[r] == 0 else 160.0 for r in rows["big"])
    assert abs(fin["nll"] - (log_loss(yt[~big], p[~big], labels=list(range(C)), normalize=False) + by_hand) / len(yt)) < 1e-9
    brier = ece_num = 0.0                                                        # a Brier score and an ECE as plain loops
    bins = [[0, 0.0, 0] for _ in range(BINS)]
    for i in range(len(yt)):
        for c in range(C):
            brier += (p[i, c] - (1.0 if c == yt[i] else 0.0)) ** 2
        conf = p[i, pred[i]]
        k = min(BINS - 1, int(conf * BINS))
        bins[k][0] += 1
        bins[k][1] += conf
        bins[k][2] += int(pred[i] == yt[i])
    for cnt, sconf, hits in bins:
        ece_num += abs(hits - sconf)
    assert abs(fin["brier"] - brier / len(yt)) < 1e-12 and abs(fin["ece"] - ece_num / len(yt)) < 1e-12
    assert [b[0] for b in bins] == state["bin_count"].tolist() and state["bin_count"].sum() == fin["n"]
    assert np.abs(bank[ok].astype(np.float64) - p).max() < 1e-7 and (bank[~ok] == 0).all() and (bank_labels[~ok] == -1).all()
    # kind "probs" on the fp32 softmax: the same integers, the sums within fp32 rounding of the probabilities
    z32 = np.where(ok[:, None], torch.softmax(torch.from_numpy(np.nan_to_num(z, posinf=0.0)), dim=1).numpy(), z)
    sp = R.new_state(C, BINS)
    R.update_ref(sp, z32.astype(np.float32), y, C, BINS, "probs")
    assert sp["n"] == state["n"] and sp["skipped"] == state["skipped"]
    assert abs(R.finish_ref(sp, C, BINS)["brier"] - fin["brier"]) < 1e-6


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("N,C", [(257, 2), (1000, 3), (255, 5)])
def test_auc_against_sklearn_and_average_ranks(N, C, quantised):
    from scipy.stats import rankdata
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(N + C)
    p = rng.random((N, C)).astype(np.float32)
    if quantised:
        p = (np.round(p * 8) / 8).astype(np.float32)                             # eighths: ties everywhere
    y = rng.integers(0, C, size=N).astype(np.int32)
    y[::17] = -1                                                                 # rows that are not used
    got = R.auc_ref(p, y, C)
    use = y >= 0
    for c in range(C):
        t, s = (y[use] == c).astype(int), p[use, c].astype(np.float64)
        assert abs(got[c, 0] - roc_auc_score(t, s)) < 1e-12
        ranks = rankdata(s)                                                      # average ranks: the Mann-Whitney U of the positives
        n_pos, n_neg = t.sum(), (1 - t).sum()
        assert abs(got[c, 0] - (ranks[t == 1].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg)) < 1e-12
        assert got[c, 1] == n_pos and got[c, 2] == n_neg and (quantised or got[c, 4] == 0)
    none = R.auc_ref(p, np.where(y == 1, 0, y).astype(np.int32), C)              # class 1 without positives; a single-class bank
    assert np.isnan(none[1, 0]) and none[1, 1] == 0
    assert np.isnan(R.auc_ref(p, np.zeros(N, np.int32), C)[:, 0]).all()


def test_segment_labels_and_pooling_restatement():
    labels = np.array([2, 2, 1, -1, 1, 0, 0, 2], np.int32)
    groups = np.array([0, 0, 1, 1, 1, 3, 3, 3], np.int32)                         # segment 2 is empty, segment 3 holds labels 0, 0, 2
    got, mixed = R.segment_labels_ref(labels, groups, 4)
    assert got.tolist() == [2, 1, -1, 0] and mixed == 1                           # (the -1 of segment 1 is no valid label: not mixed)
    src = np.arange(16, dtype=np.float32).reshape(8, 2)
    pooled = R.segment_mean_ref(src, groups, 4)
    assert pooled[2].tolist() == [0.0, 0.0] and np.allclose(pooled[1], src[2:5].mean(axis=0)) and np.allclose(pooled[3], src[5:].mean(axis=0))


# ------------------------------------------------------------------ planted defects
def test_planted_defects_change_the_result():
    rng = np.random.default_rng(3)
    p = (np.round(rng.random((257, 2)) * 8) / 8).astype(np.float32)
    y = rng.integers(0, 2, size=257).astype(np.int32)
    good, bad = R.auc_ref(p, y, 2), R.auc_ref(p, y, 2, half=False)                # `>` without the half tie
    assert good[1, 0] - bad[1, 0] > 0.04, good[1, 0] - bad[1, 0]                 # measured 0.055
    z, lab, rows = planted_case(257, 3, 11)
    a, b = R.new_state(3, BINS), R.new_state(3, BINS)
    R.update_ref(a, z, lab, 3, BINS)
    R.update_ref(b, z, lab, 3, BINS, argmax_ge=True)                              # the last index of the maximum instead of the first
    assert rows["tie"] and not np.array_equal(a["confusion"], b["confusion"])
    lab2 = np.where(lab == 2, 0, lab).astype(np.int32)                            # class 2 without support
    s = R.new_state(3, BINS)
    R.update_ref(s, z, lab2, 3, BINS)
    fin, zero = R.finish_ref(s, 3, BINS), R.finish_ref(s, 3, BINS, macro_zero=True)      # a macro mean that counts the empty class as 0
    assert np.isnan(fin["class"][2, 1]) and fin["balanced_accuracy"] - zero["balanced_accuracy"] > 0.05
    three = R.new_state(3, BINS)                                                  # batches of unequal size: batch mean != row mean
    for lo, hi in ((0, 7), (7, 200), (200, 257)):
        R.update_ref(three, z[lo:hi], lab[lo:hi], 3, BINS)
    f3 = R.finish_ref(three, 3, BINS)
    assert three["batches"] == 3 and abs(f3["val_loss"] - R.finish_ref(three, 3, BINS, row_mean_loss=True)["val_loss"]) > 1e-3
    assert abs(f3["nll"] - R.finish_ref(a, 3, BINS)["nll"]) < 1e-12 and np.array_equal(three["confusion"], a["confusion"])


def test_undefined_quantities_are_nan_in_the_restatement():
    s = R.new_state(3, BINS)
    R.update_ref(s, np.zeros((2, 3), np.float32), np.array([-1, 3], np.int32), 3, BINS)
    fin = R.finish_ref(s, 3, BINS)
    assert fin["n"] == 0 and fin["skipped"] == 2
    assert all(np.isnan(fin[k]) for k in R.SCALARS[2:]) and np.isnan(fin["class"][:, 1:]).all()


# ------------------------------------------------------------------ the binding, the refusals, the default path
NEW_SYMBOLS = ("nv_cls_metrics_state_doubles", "nv_cls_metrics_table_floats", "nv_cls_metrics_update", "nv_cls_auc_splits", "nv_cls_auc_workspace_bytes",
               "nv_cls_auc", "nv_segment_labels", "nv_cls_metrics_finish")


def test_entry_points_are_declared_bound_and_listed_in_the_makefile():
    from neurovit_amd import _cabi
    for name in NEW_SYMBOLS:
        assert name in _cabi.lib.protos, name
        assert hasattr(_cabi.lib.load(), name), name
    assert _cabi.lib.protos["nv_cls_auc_workspace_bytes"][0] is ctypes.c_long and _cabi.lib.protos["nv_cls_metrics_state_doubles"][0] is ctypes.c_long
    header = open(_cabi.HEADER).read()
    assert re.search(r"#define\s+NV_ABI_VERSION\s+8\b", header)                  # new symbols within revision 8
    for name, value in (("NV_CLS_MAX_C", _cabi.CLS_MAX_C), ("NV_CLS_MAX_BINS", _cabi.CLS_MAX_BINS), ("NV_CLS_STATE_HEAD", _cabi.CLS_STATE_HEAD),
                        ("NV_CLS_SCALARS", len(_cabi.CLS_METRIC_NAMES)), ("NV_CLS_CLASS_COLS", len(_cabi.CLS_CLASS_METRIC_NAMES)),
                        ("NV_CLS_AUC_COLS", len(_cabi.CLS_AUC_NAMES)), ("NV_CLS_AUC_MAX_SPLITS", _cabi.CLS_AUC_MAX_SPLITS)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
    assert "#define NV_CLS_AUC_MAX_N (1 << 20)" in header and _cabi.CLS_AUC_MAX_N == 1 << 20
    assert _cabi.CLS_METRIC_NAMES == R.SCALARS and _cabi.CLS_CLASS_METRIC_NAMES == R.CLASS_COLS and _cabi.CLS_STATE_NAMES == R.HEAD_NAMES
    assert _cabi.CLS_KINDS == {"logits": 0, "probs": 1}
    mk = open(os.path.join(ROOT, "neurovit_amd", "csrc", "Makefile")).read()
    assert "cls_metrics.hip" in mk.split("SRCS")[1].split("\n")[0]


def test_host_side_refusals_happen_before_any_launch():
    """bad arguments only: every call returns NV_ERR_ARG from the host-side checks, so this runs without a GPU"""
    from neurovit_amd._cabi import last_error, lib
    buf, dbuf, ibuf = (ctypes.c_float * 64)(), (ctypes.c_double * 64)(), (ctypes.c_int * 64)()
    p, d, ip = ctypes.addressof(buf), ctypes.addressof(dbuf), ctypes.addressof(ibuf)
    up = lib.nv_cls_metrics_update
    assert up(p, 4, ip, 4, 1, 15, 0, d, None, 0, None, 0, 0, None) != 0 and "C=1" in last_error()
    assert up(p, 80, ip, 4, 65, 15, 0, d, None, 0, None, 0, 0, None) != 0
    assert up(p, 4, ip, 4, 3, 0, 0, d, None, 0, None, 0, 0, None) != 0 and "bins=0" in last_error()
    assert up(p, 4, ip, 4, 3, 65, 0, d, None, 0, None, 0, 0, None) != 0
    assert up(p, 4, ip, 0, 3, 15, 0, d, None, 0, None, 0, 0, None) != 0
    assert up(p, 4, ip, 4, 3, 15, 2, d, None, 0, None, 0, 0, None) != 0 and "kind" in last_error()
    assert up(p, 2, ip, 4, 3, 15, 0, d, None, 0, None, 0, 0, None) != 0 and "lds=2" in last_error()
    assert up(p, 4, ip, 4, 3, 15, 0, d + 4, None, 0, None, 0, 0, None) != 0 and "8-byte" in last_error()
    assert up(p, 4, ip, 4, 3, 15, 0, d, p, 4, None, 0, 8, None) != 0 and "together" in last_error()
    assert up(p, 4, ip, 4, 3, 15, 0, d, p, 2, ip, 0, 8, None) != 0 and "ldb=2" in last_error()
    assert up(p, 4, ip, 4, 3, 15, 0, d, p, 4, ip, 5, 8, None) != 0 and "do not fit" in last_error()
    auc = lib.nv_cls_auc
    assert auc(p, 4, ip, 0, 3, 1, d, d, 1024, None) != 0 and auc(p, 4, ip, (1 << 20) + 1, 3, 1, d, d, 1024, None) != 0 and "N=" in last_error()
    assert auc(p, 4, ip, 8, 1, 1, d, d, 1024, None) != 0 and auc(p, 2, ip, 8, 3, 1, d, d, 1024, None) != 0 and "ldp=2" in last_error()
    assert auc(p, 4, ip, 8, 3, 257, d, d, 1024, None) != 0 and "splits" in last_error()
    assert auc(p, 4, ip, 8, 3, 1, d, d, 47, None) != 0 and "workspace" in last_error()
    assert lib.nv_cls_auc_splits(8680, 2, 0) == 17 and lib.nv_cls_auc_splits(78820, 5, 0) == 4 and lib.nv_cls_auc_splits(0, 2, 0) == 0
    assert lib.nv_cls_auc_workspace_bytes(1000, 3, 1) == 4 * 3 * 2 * 8 and lib.nv_cls_auc_workspace_bytes(1000, 3, 300) == 0
    assert lib.nv_cls_metrics_state_doubles(3, 15) == 6 + 9 + 45 and lib.nv_cls_metrics_state_doubles(65, 15) == 0
    assert lib.nv_cls_metrics_table_floats(3) == 10 + 15 + 9 and lib.nv_cls_metrics_table_floats(1) == 0
    assert lib.nv_segment_labels(ip, 4, ip, ip, 0, ip, ip, None) != 0 and lib.nv_segment_labels(ip, 4, ip, ip, 2, ip, None, None) != 0
    assert lib.nv_cls_metrics_finish(d, 1, 15, None, p, None) != 0 and lib.nv_cls_metrics_finish(d + 4, 3, 15, None, p, None) != 0


def test_host_check_program_is_clean_under_the_host_sanitizers():
    """tools/cls_metrics_host_check.cpp: the new host entry points (argument checks, sizing) in a stand-alone program built with
    -Xarch_host -fsanitize=address,undefined; it makes bad-argument calls only, so nothing is launched.  Nothing loaded into Python is sanitised."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "neurovit_amd", "csrc"), "cls-metrics-host-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    both = out.stdout + out.stderr
    assert "cls_metrics_host_check: ok" in out.stdout and "runtime error" not in both and "AddressSanitizer" not in both


def test_python_refusals_without_a_device():
    from neurovit_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ClassificationMetrics(3, device="cpu")
    for bad in (dict(num_classes=1), dict(num_classes=65), dict(num_classes=3, bins=0), dict(num_classes=3, bins=65), dict(num_classes=3, capacity=-1),
                dict(num_classes=3, capacity=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            ops.ClassificationMetrics(**bad)
    m = object.__new__(ops.ClassificationMetrics)                                 # the checks of update() run in front of any device call
    m.C, m.capacity, m.bins, m.size = 3, 0, 15, 0
    y = torch.zeros(4, dtype=torch.int64)
    for scores in (torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 2), torch.zeros(12), [[0.0] * 3] * 4):
        with pytest.raises(ValueError, match="scores"):                          # a CPU tensor, a wrong dtype, width, rank, no tensor at all
            m.update(scores, y)
    with pytest.raises(ValueError, match="kind"):
        m.update(torch.zeros(4, 3), y, kind="softmax")


SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=1, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=64)


def test_config_key_is_checked_and_the_default_path_is_untouched():
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd import trainer as T
    parse = T.Trainer.metrics_from_config
    assert parse({}) is None and parse({"VALIDATION_METRICS": None}) is None and parse({"VALIDATION_METRICS": False}) is None
    assert parse({"VALIDATION_METRICS": True}) == dict(bins=15, subject_index=0)
    assert parse({"VALIDATION_METRICS": True, "VALIDATION_CALIBRATION_BINS": 10, "VALIDATION_SUBJECT_INDEX": 1}) == dict(bins=10, subject_index=1)
    with pytest.warns(UserWarning, match="unweighted"):                           # val_loss leaves the class weights out: said at configuration time
        assert parse({"VALIDATION_METRICS": True, "TRAINING_CLASS_WEIGHTS": [1.0, 2.0]}) == dict(bins=15, subject_index=0)
    for objective in ("regression", "mim"):
        with pytest.raises(ValueError, match="VALIDATION_METRICS"):
            parse({"VALIDATION_METRICS": True, "TRAINING_OBJECTIVE": objective})
    for bad in ({"VALIDATION_CALIBRATION_BINS": 0}, {"VALIDATION_CALIBRATION_BINS": 65}, {"VALIDATION_CALIBRATION_BINS": 1.5}, {"VALIDATION_CALIBRATION_BINS": True},
                {"VALIDATION_SUBJECT_INDEX": "0"}):
        with pytest.raises(ValueError):
            parse(dict(bad, VALIDATION_METRICS=True))
    # no key: the objective is _Supervised itself, whose validation methods are the ones of the class (nothing wrapped, nothing replaced)
    cfg = dict(W.neuro_config(12, 3, DEVICE="cpu", **SIZE), GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=2, TRAINING_NUM_WORKERS=0,
               TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2)
    ds = torch.utils.data.TensorDataset(torch.arange(4), torch.zeros(4, 1), torch.zeros(4, 12, 12, 12), torch.tensor([0, 1, 0, 1]))
    plain = T.Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
    assert type(plain.objective) is T._Supervised and plain.validation_metrics is None and not plain.objective.wants_subjects
    measured = T.Trainer(dict(cfg, VALIDATION_METRICS=True), ne.NeuroEncoder(cfg), ds, ds)
    assert type(measured.objective) is T._Measured and measured.objective.wants_subjects
    for name in ("batch", "report", "begin"):
        assert getattr(T._Measured, name) is not getattr(T._Supervised, name)
    for name in ("train_batch", "update", "statistic", "sample", "samples", "begin_samples", "unpack", "make_step"):      # training and evaluate_samples: shared
        assert getattr(T._Measured, name) is getattr(T._Supervised, name)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                    # the metrics run on the device only
        measured.validate(0)
    with pytest.raises(ValueError, match="VALIDATION_METRICS"):
        T.Trainer(dict(cfg, VALIDATION_METRICS=True, TRAINING_OBJECTIVE="mim"), ne.NeuroEncoder(cfg), ds, ds)
    assert T.Trainer._batch_subjects([["a", "b"], 0, 1]) == ["a", "b"] and T.Trainer._batch_subjects([torch.zeros(2), 0, 1]) is None
    assert T.Trainer._batch_subjects([0, torch.tensor([3, 4]), 1], 1).tolist() == [3, 4] and T.Trainer._batch_subjects([torch.zeros(2), 0]) is None
