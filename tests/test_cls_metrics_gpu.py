"""The classification metrics on the MI355X (nv_cls_metrics_update / nv_cls_auc / nv_segment_labels / nv_cls_metrics_finish and
ops.ClassificationMetrics) held to the float64 restatement (tests/cls_metrics_ref.py; what it is worth is proven in
tests/test_cls_metrics_cpu.py), and the Trainer's VALIDATION_METRICS pass.

Gates: every integer quantity (n, skipped, confusion matrix, bin counts, gt / eq, n_pos / n_neg, mixed, subject labels) exact; AUC bit-equal
to the double quotient of those integers at every split count; bank probabilities within one fp32 ulp of float32(float64 softmax) (double
rounding can flip the last bit); double sums within SUM_GATE = 1e-9 (absolute on quantities of order 1, relative above: at most ~1e3 * C
terms with a few ulp of 2.2e-16 each); the fp32 finish table within FP32_GATE = 1.2e-7 (one fp32 ulp) of the restated value.
Measured maxima on the MI355X (every figure is printed in front of its gate: run with -s): bank probabilities 0 ulp under both kinds;
double sums 9.5e-16 (update, logits), 5.5e-16 (probs), 4.1e-16 (three updates), 3.2e-16 / 1.5e-16 (volumes / subjects of the pooling
case), 0 (subjects with skipped rows); finish table 5.7e-8 (both kinds), 3.8e-8 (subjects); all integer quantities and every AUC bit exact."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cls_metrics_ref as R
import weights as W

pytestmark = pytest.mark.gpu

BINS = 15


def note(name, value):
    """every figure is printed in front of its gate (run with -s); the maxima of a run are in the module's docstring and in the README"""
    print(f"measured {name}: {float(value):.3e}")


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def sum_err(got, want):
    """The error of double sums under SUM_GATE = 1e-9: |got - want| / max(1, |want|), i.e. the ABSOLUTE error for a quantity of order 1 (the
    means and every finished metric) and the RELATIVE error for a raw sum above 1 (nll_sum reaches 3e2 here, where an absolute 1e-9 would ask
    for 3e-12 relative - still met: the measured maxima are below 1e-15 under either reading).  Equal infinities (the nll of a zero
    probability) agree."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.where(got == want, 0.0, np.abs(got - want) / np.maximum(1.0, np.abs(want)))
    assert not np.isnan(err).any(), (got, want)
    return float(err.max()) if err.size else 0.0


def table_err(got, want):
    """fp32 table against the restated float64 values: NaN exactly where the restatement has NaN, else the relative error"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    keep = ~np.isnan(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(got[keep] == want[keep], 0.0, np.abs(got[keep] - want[keep]) / np.abs(want[keep]))
    return float(err.max()) if err.size else 0.0


def ulps(got, want64):
    """the distance of fp32 values from float32(want64) in fp32 ulps of the wanted value"""
    want = want64.astype(np.float32)
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


def same_doubles(got, want):
    """NaN at the same places, equal bits elsewhere"""
    keep = ~np.isnan(want)
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[keep].view(np.int64), want[keep].view(np.int64))


def state_of(m, state=None):
    parts = {k: host(v) for k, v in m.state_parts(state).items()}
    return dict(zip(R.HEAD_NAMES, parts.pop("head")), **parts)


def hold_state(got, want, what):
    """integer parts exact, double sums within SUM_GATE"""
    for key in ("n", "skipped", "batches"):
        assert got[key] == want[key], (what, key, got[key], want[key])
    for key in ("confusion", "bin_count", "bin_correct"):
        assert np.array_equal(got[key], want[key].astype(np.float64)), (what, key)
    err = max(sum_err([got[k] for k in ("nll_sum", "batch_mean_sum", "brier_sum")], [want[k] for k in ("nll_sum", "batch_mean_sum", "brier_sum")]),
              sum_err(got["bin_conf"], want["bin_conf"]))
    note(f"{what}: double sums", err)
    assert err <= R.SUM_GATE, (what, err)


def raw_update(ops, scores, labels, C, kind, state, bank=None, bank_labels=None, row0=0, capacity=0):
    from neurovit_amd._cabi import CLS_KINDS, check, lib
    check(lib.nv_cls_metrics_update(scores.data_ptr(), scores.stride(0), labels.data_ptr(), scores.shape[0], C, BINS, CLS_KINDS[kind], state.data_ptr(),
                                    None if bank is None else bank.data_ptr(), 0 if bank is None else bank.stride(0),
                                    None if bank_labels is None else bank_labels.data_ptr(), row0, capacity, torch.cuda.current_stream().cuda_stream),
          "nv_cls_metrics_update")


def planted_case(B, C):
    z, y = R.logits_case(B, C, 100 * B + C)
    rows = R.plant(z, y, C)
    assert R.check_inputs(z, y, C, BINS, "logits") == rows["tie"]
    return z, y, rows


# ------------------------------------------------------------------ update / finish
@pytest.mark.parametrize("B", [1, 7, 256, 257])
@pytest.mark.parametrize("C", [2, 3, 5])
def test_update_and_finish_against_the_restatement_with_guard_cells(ops, B, C):
    """lds = C + 3 with NaN guard cells around the rows, a bank window of leading dimension C + 3 inside a NaN-filled bank; labels -1 and C,
    NaN / inf logits, an exact tie, logits of +-80; kind "logits", then kind "probs" on the fp32 softmax of the same logits"""
    from neurovit_amd._cabi import check, lib
    z, y, rows = planted_case(B, C)
    z32 = np.where(R.valid_rows(z, y, C)[:, None], torch.softmax(torch.from_numpy(np.nan_to_num(z, posinf=0.0)), dim=1).numpy(), z).astype(np.float32)
    for kind, scores in (("logits", z), ("probs", z32)):
        assert R.check_inputs(scores, y, C, BINS, kind) == rows["tie"]
        want = R.new_state(C, BINS)
        want_bank, want_labels = R.update_ref(want, scores, y, C, BINS, kind)
        buf = torch.full((B + 2, C + 3), float("nan"), device="cuda")
        buf[1:B + 1, :C] = dev(scores)
        cap, row0 = B + 5, 2
        bank = torch.full((cap, C + 3), float("nan"), device="cuda")
        bank_labels = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
        state = torch.zeros(lib.nv_cls_metrics_state_doubles(C, BINS), dtype=torch.float64, device="cuda")
        m = ops.ClassificationMetrics(C, bins=BINS)
        raw_update(ops, buf[1:B + 1, :C], dev(y), C, kind, state, bank, bank_labels, row0, cap)
        hold_state(state_of(m, state), want, f"update {kind}")
        # the bank window: float(p) within an ulp, zeros and -1 on the skipped rows, every guard cell untouched
        got_bank, got_labels = host(bank), host(bank_labels)
        window = got_bank[row0:row0 + B, :C]
        ok = R.valid_rows(scores, y, C)
        assert np.array_equal(got_labels[row0:row0 + B], want_labels) and (window[~ok] == 0).all()
        if ok.any():
            d = ulps(window[ok], R.probabilities(scores, kind)[ok])
            note(f"bank {kind}: ulps", d)
            assert d <= 1.0
        assert np.isnan(got_bank[:row0]).all() and np.isnan(got_bank[row0 + B:]).all() and np.isnan(got_bank[:, C:]).all()
        assert (got_labels[:row0] == -7).all() and (got_labels[row0 + B:] == -7).all() and np.isnan(host(buf)[:, C:]).all()
        # finish (no AUC table: the AUC cells are NaN)
        table = torch.full((lib.nv_cls_metrics_table_floats(C) + 2,), 7.0, device="cuda")
        check(lib.nv_cls_metrics_finish(state.data_ptr(), C, BINS, None, table[1:].data_ptr(), torch.cuda.current_stream().cuda_stream), "nv_cls_metrics_finish")
        got = host(table)
        assert got[0] == 7.0 and got[-1] == 7.0
        err = table_err(got[1:-1], R.table_ref(R.finish_ref(want, C, BINS), C))
        note(f"finish {kind}: table", err)
        assert err <= R.FP32_GATE


def test_split_batches_equal_the_whole_in_every_integer_and_two_runs_in_every_bit(ops):
    C, B = 3, 257
    z, y, rows = planted_case(B, C)
    cuts = [(0, 7), (7, 200), (200, 257)]
    runs = []
    for _ in range(2):
        whole, split = ops.ClassificationMetrics(C, capacity=B, bins=BINS), ops.ClassificationMetrics(C, capacity=B, bins=BINS)
        whole.update(dev(z), dev(y))
        for lo, hi in cuts:
            split.update(dev(z[lo:hi]), dev(y[lo:hi]))
        runs.append((whole, split, whole.compute_device(), split.compute_device()))
    (whole, split, dw, ds), (whole2, split2, dw2, ds2) = runs
    sw, ss = state_of(whole), state_of(split)
    for key in ("n", "skipped"):
        assert sw[key] == ss[key]
    for key in ("confusion", "bin_count", "bin_correct"):
        assert np.array_equal(sw[key], ss[key])
    assert sw["batches"] == 1 and ss["batches"] == 3
    assert torch.equal(whole.bank_probs, split.bank_probs) and torch.equal(whole.bank_labels, split.bank_labels)      # a row's terms do not depend on its batch
    assert torch.equal(dw["auc"], ds["auc"])
    err = max(sum_err([ss[k] for k in ("nll_sum", "brier_sum")], [sw[k] for k in ("nll_sum", "brier_sum")]), sum_err(ss["bin_conf"], sw["bin_conf"]))
    note("split against whole: double sums", err)
    assert err <= R.SUM_GATE
    # val_loss differs by definition (the mean of three batch means): against the restatement
    want = R.new_state(C, BINS)
    for lo, hi in cuts:
        R.update_ref(want, z[lo:hi], y[lo:hi], C, BINS)
    hold_state(ss, want, "three updates")
    fin = R.finish_ref(want, C, BINS, R.auc_ref(host(split.bank_probs), host(split.bank_labels), C))
    assert table_err(host(ds["table"]), R.table_ref(fin, C)) <= R.FP32_GATE
    got, one = split.compute(), whole.compute()
    assert abs(got["val_loss"] - fin["val_loss"]) <= R.FP32_GATE * abs(fin["val_loss"]) and abs(got["val_loss"] - one["val_loss"]) > 1e-3
    assert abs(one["val_loss"] - one["nll"]) <= 1e-6 * one["nll"]
    # two runs: every bit of the states and of the tables (NaN cells included)
    for a, b in ((whole, whole2), (split, split2)):
        assert torch.equal(a.state, b.state)
    for a, b in ((dw, dw2), (ds, ds2)):
        assert torch.equal(a["table"].view(torch.int32), b["table"].view(torch.int32)) and torch.equal(a["auc"].view(torch.int64), b["auc"].view(torch.int64))


def test_undefined_quantities_are_nan(ops):
    m = ops.ClassificationMetrics(3, capacity=4, bins=BINS)
    m.update(torch.zeros(2, 3, device="cuda"), torch.tensor([-1, 3]))                        # n = 0: every row skipped
    got = m.compute()
    assert got["n"] == 0 and got["skipped"] == 2 and got["confusion"].sum() == 0
    for key in ("accuracy", "balanced_accuracy", "macro_f1", "nll", "val_loss", "brier", "ece", "macro_auc"):
        assert math.isnan(got[key]), key
    assert torch.isnan(got["class_recall"]).all() and torch.isnan(got["class_precision"]).all() and torch.isnan(got["class_auc"]).all()
    m.reset()
    z = torch.tensor([[3.0, 0.0, -1.0], [2.0, 1.0, 0.0], [0.0, 4.0, 1.0]], device="cuda")     # class 2 is never predicted and has no support
    m.update(z, torch.tensor([0, 1, 1]))
    got = m.compute()
    assert got["n"] == 3 and got["confusion"].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 0]]
    assert math.isnan(float(got["class_precision"][2])) and math.isnan(float(got["class_recall"][2])) and math.isnan(float(got["class_f1"][2]))
    assert math.isnan(float(got["class_auc"][2])) and float(got["class_recall"][1]) == 0.5 and float(got["class_precision"][0]) == 0.5
    assert abs(got["balanced_accuracy"] - 0.75) < 1e-7 and not math.isnan(got["macro_auc"])      # the means run over the defined classes only
    plain = ops.ClassificationMetrics(2, bins=BINS)                                            # no bank: no AUC keys, and the two-class extras
    plain.update(torch.tensor([[1.0, 0.0], [0.0, 2.0], [1.0, 0.5]], device="cuda"), torch.tensor([0, 1, 1]))
    got = plain.compute()
    assert "auc" not in got and "macro_auc" not in got and got["sensitivity"] == 0.5 and got["specificity"] == 1.0
    with pytest.raises(ValueError, match="capacity"):
        m.update(torch.zeros(2, 3, device="cuda"), torch.tensor([0, 1]))                      # 3 + 2 rows in a bank of 4
    with pytest.raises(ValueError, match="groups"):
        plain.update(torch.zeros(2, 2, device="cuda"), torch.tensor([0, 1]), groups=[0, 1])


# ------------------------------------------------------------------ AUC
def auc_case(N, C, quantised, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((N, C)).astype(np.float32)
    if quantised:
        p = (np.round(p * 8) / 8).astype(np.float32)
    y = rng.integers(0, C, size=N).astype(np.int32)
    y[3::11] = -1
    y[5::13] = C + (np.arange(len(y[5::13])) % 2)                                                      # labels C and C + 1: not used either
    return p, y


@pytest.mark.parametrize("quantised", [True, False])
@pytest.mark.parametrize("N,C", [(1, 3), (2, 3), (255, 3), (256, 2), (257, 5), (1000, 3), (300, 33), (300, 64)])
def test_auc_counts_are_exact_at_every_split(ops, N, C, quantised):
    """dense (16-byte loads) and with a padded leading dimension; C = 33 / 64: the tiles of 248 / 128 rows"""
    p, y = auc_case(N, C, quantised, 7 * N + C)
    want = R.auc_ref(p, y, C)
    padded = torch.full((N, C + 3), float("nan"), device="cuda")
    padded[:, :C] = dev(p)
    for splits in (1, 3, 0):
        for probs in (dev(p), padded[:, :C]):
            got = host(ops.cls_auc(probs, dev(y), splits=splits))
            assert np.array_equal(got[:, 1:], want[:, 1:]), (splits, got[:, 1:], want[:, 1:])            # n_pos, n_neg, gt, eq
            assert same_doubles(got[:, 0], want[:, 0]), (splits, got[:, 0], want[:, 0])                  # the double quotient of those integers, bit for bit
    if quantised and N >= 255 and C <= 5:
        assert want[:, 4].min() > 0                                                                     # ties everywhere


def test_auc_is_nan_without_positives_or_negatives(ops):
    p, y = auc_case(257, 3, True, 5)
    y0 = np.where(y == 1, 0, y).astype(np.int32)                                                       # class 1 without positives
    got, want = host(ops.cls_auc(dev(p), dev(y0))), R.auc_ref(p, y0, 3)
    assert np.isnan(got[1, 0]) and got[1, 1] == 0 and np.array_equal(got[:, 1:], want[:, 1:]) and got[0, 0] == want[0, 0] and got[2, 0] == want[2, 0]
    single = host(ops.cls_auc(dev(p), torch.zeros(257, dtype=torch.int32, device="cuda")))            # a single-class bank
    assert np.isnan(single[:, 0]).all() and single[0, 1] == 257 and single[0, 2] == 0 and (single[:, 3:] == 0).all()
    unused = host(ops.cls_auc(dev(p), torch.full((257,), -1, dtype=torch.int32, device="cuda")))
    assert np.isnan(unused[:, 0]).all() and (unused[:, 1:] == 0).all()


# ------------------------------------------------------------------ subject pooling
def test_subject_pooling_against_the_restatement(ops):
    """subjects of 1, 2 and 300 rows, an empty segment (id 3), a subject with mixed labels (id 4), one more (id 5); batches of 64 rows"""
    C = 3
    sizes, subject_label = [1, 2, 300, 0, 5, 4], [0, 1, 2, -1, 1, 0]
    groups = np.concatenate([np.full(n, g, np.int32) for g, n in enumerate(sizes)])
    labels = np.concatenate([np.full(n, subject_label[g], np.int32) for g, n in enumerate(sizes)])
    labels[np.nonzero(groups == 4)[0][2]] = 2                                                          # the mixed subject: 1, 1, 2, 1, 1
    rng = np.random.default_rng(9)
    perm = rng.permutation(len(groups))                                                                 # the subjects' rows lie scattered over the batches
    groups, labels = groups[perm], labels[perm]
    N = len(groups)
    z = (2.0 * rng.standard_normal((N, C))).astype(np.float32)
    z[np.arange(N), labels] += 1.5
    assert R.check_inputs(z, labels, C, BINS, "logits") == []
    m = ops.ClassificationMetrics(C, capacity=N + 3, bins=BINS)
    batches = [(z[i:i + 64], labels[i:i + 64]) for i in range(0, N, 64)]
    for i, (s, l) in enumerate(batches):
        m.update(dev(s), dev(l), groups=groups[64 * i:64 * i + 64])
    d = m.compute_device()
    bank, bank_labels = host(m.bank_probs[:N]), host(m.bank_labels[:N])
    fin, sub, extra = R.compute_ref(batches, C, BINS)                                                   # the restated bank: within an ulp of the device's
    assert np.array_equal(bank_labels, extra["bank_labels"]) and ulps(bank, extra["bank"].astype(np.float64)) <= 1.0
    fin, sub, extra = R.compute_ref(batches, C, BINS, groups=groups, bank=(bank, bank_labels))          # pooled from the device's own bank: the same bits
    hold_state(state_of(m), extra["state"], "volumes")
    assert np.array_equal(host(d["auc"])[:, 1:], extra["auc"][:, 1:]) and np.array_equal(host(d["auc"])[:, 0], extra["auc"][:, 0])
    assert table_err(host(d["table"]), R.table_ref(fin, C)) <= R.FP32_GATE
    assert host(d["subject_labels"]).tolist() == [0, 1, 2, -1, 1, 0] == extra["subject_labels"].tolist()
    assert int(d["subject_mixed"]) == 1 == extra["subject_mixed"]
    assert np.array_equal(host(d["subject_probs"]), extra["subject_probs"]) and (host(d["subject_probs"])[3] == 0).all()
    hold_state(state_of(m, d["subject_state"]), extra["subject_state"], "subjects")
    assert extra["subject_state"]["n"] == 5 and extra["subject_state"]["skipped"] == 1                  # the empty segment is skipped and counted
    assert np.array_equal(host(d["subject_auc"])[:, 1:], extra["subject_auc"][:, 1:]) and np.array_equal(host(d["subject_auc"])[:, 0], extra["subject_auc"][:, 0])
    err = table_err(host(d["subject_table"]), R.table_ref(sub, C))
    note("subject table", err)
    assert err <= R.FP32_GATE
    got = m.compute()
    assert got["subject_mixed_labels"] == 1 and got["subject_n"] == 5 and got["subject_confusion"].sum() == 5 and got["n"] == N
    assert abs(got["subject_macro_auc"] - sub["macro_auc"]) <= R.FP32_GATE * sub["macro_auc"]
    assert abs(got["subject_balanced_accuracy"] - sub["balanced_accuracy"]) <= R.FP32_GATE * sub["balanced_accuracy"]
    # segment_labels alone, a bank label of -1 in a segment is no second label
    lab = torch.tensor([2, -1, 2, 1, 0, 7, 7, -1, 1], dtype=torch.int32, device="cuda")               # (a label >= C is a label like any other here)
    out, mixed = ops.segment_labels(lab, *ops.segment_csr([0, 0, 0, 1, 1, 2, 2, 3, 3]))
    assert out.tolist() == [2, 1, 7, -1] and int(mixed) == 2                                            # segment 3: first row -1, then a valid label


def test_a_skipped_row_inside_a_subject_is_pooled_as_zeros(ops):
    """The documented consequence of filing a skipped row as zeros with label -1: it stays in its subject's mean, so one
    NaN volume of k scales the subject's probabilities by (k - 1) / k; a subject whose FIRST row is skipped gets label -1, is skipped as a
    whole and counted in subject_mixed_labels.  Held to the restatement, which follows the same rule."""
    C = 3
    z = np.array([[2.0, 0.0, -1.0], [0.5, np.nan, 0.0], [1.5, 0.5, -0.5], [np.inf, 0.0, 0.0], [0.0, 3.0, 1.0], [0.0, 2.0, 1.0]], np.float32)
    y = np.array([0, 0, 0, 1, 1, 1], np.int32)
    groups = np.array([0, 0, 0, 1, 1, 1], np.int32)
    m = ops.ClassificationMetrics(C, capacity=6, bins=BINS)
    m.update(dev(z), dev(y), groups=groups)
    d = m.compute_device()
    bank, bank_labels = host(m.bank_probs), host(m.bank_labels)
    assert bank_labels.tolist() == [0, -1, 0, -1, 1, 1] and (bank[[1, 3]] == 0).all()
    fin, sub, extra = R.compute_ref([(z, y)], C, BINS, groups=groups, bank=(bank, bank_labels))
    pooled = host(d["subject_probs"])
    assert np.array_equal(pooled, extra["subject_probs"]) and abs(pooled[0].sum() - 2.0 / 3.0) < 1e-6 and abs(pooled[1].sum() - 2.0 / 3.0) < 1e-6
    assert host(d["subject_labels"]).tolist() == [0, -1] == extra["subject_labels"].tolist() and int(d["subject_mixed"]) == 1 == extra["subject_mixed"]
    hold_state(state_of(m, d["subject_state"]), extra["subject_state"], "subjects with skipped rows")
    assert extra["subject_state"]["n"] == 1 and extra["subject_state"]["skipped"] == 1
    assert table_err(host(d["subject_table"]), R.table_ref(sub, C)) <= R.FP32_GATE
    # a caller who knows the bad rows on the host gives them group -1: they are in no subject
    m.reset()
    m.update(dev(z), dev(y), groups=np.array([0, -1, 0, -1, 1, 1], np.int32))
    d = m.compute_device()
    pooled = host(d["subject_probs"])
    assert np.abs(pooled.sum(axis=1) - 1.0).max() < 1e-6 and host(d["subject_labels"]).tolist() == [0, 1] and int(d["subject_mixed"]) == 0
    assert state_of(m, d["subject_state"])["n"] == 2 and state_of(m, d["subject_state"])["skipped"] == 0


# ------------------------------------------------------------------ the Trainer
SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
READS = ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__")


class Planted(torch.utils.data.Dataset):
    """n volumes +-pattern + noise, label = the sign, four volumes per subject NAME, as 4-tuples (subject, a number, the volume, the label)"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        pattern = torch.randn(32, 32, 32, generator=torch.Generator().manual_seed(99))
        self.labels = (torch.arange(n) // 4) % 2                                                       # a subject's volumes share its label
        self.vol = (self.labels.float() * 2 - 1)[:, None, None, None] * pattern + 0.3 * torch.randn(n, 32, 32, 32, generator=g)

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return f"sub-{i // 4:03d}", float(i), self.vol[i], self.labels[i]


def trainer_config(**extra):
    return dict(W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **SIZE),
                GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=2, TRAINING_BATCH_SIZE=4, TRAINING_NUM_WORKERS=0, **extra)


def spy_on_reads(monkeypatch, reads):
    for name in READS:
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)


def test_trainer_reports_device_metrics_only_when_asked(ops, monkeypatch, capsys):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer, _Measured, _Supervised
    torch.manual_seed(5)
    cfg = trainer_config(VALIDATION_METRICS=True, TRAINING_EMA_DECAY=0.5, VALIDATION_PRECISION="bf16")
    model = ne.NeuroEncoder(cfg)
    t = Trainer(cfg, model, Planted(40, 1), Planted(12, 2))
    assert type(t.objective) is _Measured
    logged = []
    t._log = logged.append
    first_loss, before = t.validate(-1)
    for epoch in range(2):
        t.train(epoch)
    capsys.readouterr()
    reads = []
    spy_on_reads(monkeypatch, reads)
    t.validate_ema = False
    logged.clear()
    loss, after = t.validate(1)
    monkeypatch.undo()
    assert reads == ["cpu"], reads                                                                      # one host read for a whole validation pass
    print(f"planted classes: validation loss {first_loss:.4f} -> {loss:.4f}, accuracy {before:.3f} -> {after:.3f} over two epochs")
    assert loss < first_loss and after >= before                                                        # the planted classes are learned
    C, got = t.metrics.C, t.val_metrics
    keys = ["val_loss", "val_accuracy", "val_balanced_accuracy", "val_macro_f1", "val_auc", "val_nll", "val_brier", "val_ece"]
    keys += ["val_sensitivity", "val_specificity"] if C == 2 else []
    keys += ["val_subject_accuracy", "val_subject_balanced_accuracy", "val_subject_auc"]
    assert len(logged) == 1 and list(logged[0]) == ["epoch"] + keys, logged
    line = capsys.readouterr().out
    assert all(f"{k} " in line for k in keys)
    assert got["confusion"].shape == (C, C) and int(got["confusion"].sum()) == 12 == got["n"] and got["subject_n"] == 3 and got["subject_mixed_labels"] == 0
    assert int(got["subject_confusion"].sum()) == 3 and t.val_loss == logged[0]["val_loss"] == loss
    # the logged numbers are ClassificationMetrics over the same batches, and val_loss is the reference's: the mean of the batches' criterion
    met = ops.ClassificationMetrics(C, capacity=12)
    model.eval()
    total, hits = 0.0, 0
    with torch.no_grad(), model.precision(t.validation_precision):
        for batch in t.val_dataloader:
            out = model(batch[2].cuda()).float()
            met.update(out, batch[-1])
            total += t.criterion(out, batch[-1].cuda()).item()
            hits += (out.argmax(dim=1).cpu() == batch[-1]).sum().item()
    want = met.compute()
    assert torch.equal(want["confusion"], got["confusion"]) and want["nll"] == got["nll"] and want["macro_auc"] == got["macro_auc"]
    assert abs(loss - round(total / len(t.val_dataloader), 5)) < 2e-5 and after == round(hits / 12, 5)
    # the weight average is validated behind the model and tagged
    t.validate_ema = True
    logged.clear()
    t.validate(1)
    assert len(logged) == 2 and list(logged[1]) == ["epoch"] + [k + "_ema" for k in keys] and t.val_metrics_ema["n"] == 12
    assert "val_auc_ema" in capsys.readouterr().out
    # without the key: the reference's pass - the printed line and the logged keys are exactly what they were
    plain_cfg = trainer_config()
    plain = Trainer(plain_cfg, ne.NeuroEncoder(plain_cfg), Planted(8, 3), Planted(8, 4))
    assert type(plain.objective) is _Supervised and not hasattr(plain, "metrics")
    logged.clear()
    plain._log = logged.append
    capsys.readouterr()
    loss, accuracy = plain.validate(0)
    assert logged == [{"epoch": 0, "val_loss": loss, "val_accuracy": accuracy}]
    assert capsys.readouterr().out == f"[VALIDATION] epoch 0\t| total_batch 1\t| val_loss {loss:.5f}\t| val_accuracy {accuracy:.5f}\n"
    assert not hasattr(plain, "val_metrics")
