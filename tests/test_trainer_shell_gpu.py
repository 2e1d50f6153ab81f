"""The Trainer shell's one training loop under each objective, and the one scorer behind knn_evaluate / linear_evaluate.

The loop: the host reads the device at a log line and nowhere else.  The expectation is the shell's as it stood before the three loops became
one (tools/trainer_transcript.py records it per batch, profiles/trainer_shell_refactor.txt): float(running_loss), then float(correct) or
float(abs_err) and int(seen), then float(last_grad_norm) when the step clips - all inside the log branch.
The scorer: mae / subject_mae and acc / subject_acc against a float64 restatement on hand-made features, no encoder."""
import math

import pytest
import torch

import weights as W

pytestmark = pytest.mark.gpu

SIZE = dict(TRAINING_VIT_DIM=128, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=2, TRAINING_VIT_MLP_DIM=256)
READS = ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__")


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import ops
    return ops


def volumes(n, seed):
    """n 32^3 volumes as 7-tuples in the ADNI order: the volume is element 2, `age` element -2, the label the last"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(n, generator=g) * 2 - 1
    ids = torch.arange(n)
    return torch.utils.data.TensorDataset(ids, ids.clone(), W.make_volume((n, 32, 32, 32), seed) * (1 + 0.5 * a[:, None, None, None]), ids.clone(),
                                          ids.clone(), 70.0 + 8.0 * a, (a > 0).long())


OBJECTIVES = {
    "supervised": (dict(TRAINING_GRAD_CLIP=1.0, AUGMENT_MIXUP_ALPHA=0.4), ["__float__", "__float__", "__float__"]),        # loss, correct, grad norm
    "regression": (dict(TRAINING_OBJECTIVE="regression", REGRESSION_TARGET_MEAN=[70.0], REGRESSION_TARGET_STD=[8.0], AUGMENT_MIXUP_ALPHA=0.4),
                   ["__float__", "__float__", "__int__"]),                                                                  # loss, abs_err, seen
    "mim": (dict(TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.5), ["__float__"]),                                        # loss
}


@pytest.mark.parametrize("objective", list(OBJECTIVES))
def test_train_reads_the_device_only_at_log_lines(ops, monkeypatch, objective):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer
    extra, at_a_log_line = OBJECTIVES[objective]
    cfg = dict(W.neuro_config(32, 8, DEVICE="cuda", TRAINING_LEARNING_RATE=1e-3, TRAINING_WEIGHT_DECAY=1e-2, **SIZE, **extra),
               GLOBAL_OUTPUT_DIR="unused", TRAINING_EPOCHS=1, TRAINING_BATCH_SIZE=4, TRAINING_NUM_WORKERS=0)
    torch.manual_seed(21)
    t = Trainer(cfg, ne.NeuroEncoder(cfg), volumes(24, 1), volumes(8, 2))
    t.log_interval = 2                                            # 6 batches: log lines at i = 2 and 4; 0, 1, 3 and 5 must stay on the device
    batches, unpack = [], t._unpack

    def begin_batch(batch):                                      # every batch of the loop begins here
        batches.append([])
        return unpack(batch)
    t._unpack = begin_batch
    for name in READS:
        real = getattr(torch.Tensor, name)

        def spy(self, *a, _real=real, _name=name, **k):
            if self.is_cuda and batches:
                batches[-1].append(_name)
            return _real(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    t.train(0)
    monkeypatch.undo()
    print(f"{objective}: reads per batch {batches}")
    assert len(batches) == 6 and t.global_step == 6
    for i, reads in enumerate(batches):
        assert reads == (at_a_log_line if i in (2, 4) else []), (i, reads)


# ------------------------------------------------------------------ the scorer
GROUPS = torch.tensor([0, 1, 1, 2, 2, 2, 2])                     # Nq = 7 queries: three subjects of 1, 2 and 4 volumes


def features(n, seed):
    x = torch.randn(n, 8, generator=torch.Generator().manual_seed(seed))
    return (x / x.norm(dim=1, keepdim=True)).cuda()


def subject_means(values):
    """float64 [G, K]: the mean of each subject's cells that are not NaN, NaN where it has none"""
    rows = []
    for g in range(int(GROUPS.max()) + 1):
        v = values[GROUPS == g]
        seen = ~torch.isnan(v)
        rows.append(torch.where(seen, v, torch.zeros_like(v)).sum(0) / seen.sum(0))          # 0 / 0 = NaN: nothing observed
    return torch.stack(rows)


def mae64(pred, target):
    """float64 restatement: the mean absolute error of each column over its observed cells (NaN for a column without one)"""
    seen = ~torch.isnan(target)
    return (torch.where(seen, (pred - target).abs(), torch.zeros_like(target)).sum(0) / seen.sum(0)).tolist()


def close(got, want):
    """rtol 1e-5 (the tolerance tests/test_probe_gpu.py holds `mae` to); NaN where the restatement has NaN"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-5 * abs(w), (got, want)


def test_probe_scorers_agree_with_a_float64_restatement(ops):
    from neurovit_amd import FeatureBank, LinearProbe, knn_evaluate, linear_evaluate
    X, Q = features(12, 31), features(7, 32)
    bank_targets = torch.randn(12, 2, generator=torch.Generator().manual_seed(33)) * torch.tensor([8.0, 2.0]) + torch.tensor([20.0, 5.0])
    T = torch.randn(7, 2, generator=torch.Generator().manual_seed(34)) * torch.tensor([8.0, 2.0]) + torch.tensor([20.0, 5.0])
    T[3, 0] = float("nan")                                        # one missing cell
    T[1:3, 1] = float("nan")                                      # subject 1 has no observed second target
    bank = FeatureBank.from_features(X, targets=bank_targets, groups=torch.arange(12) + 3)      # (no bank row shares a subject with a query)
    probe = LinearProbe(8, num_targets=2, l2=[1e-3, 0.1]).fit(bank, steps=20)
    # a column with nothing observed at all: its mae and subject_mae are NaN (nv_reg_metrics_finish: n = 0), the other column is unaffected -
    # what the evaluators returned before they shared the scorer
    for targets, empty in ((T, False), (torch.stack([T[:, 0], torch.full((7,), float("nan"))], dim=1), True)):
        t64 = targets.double()
        knn = knn_evaluate(bank, Q, targets=targets, k=(1, 3), query_groups=GROUPS)
        lin = linear_evaluate(probe, Q, targets=targets, query_groups=GROUPS)
        assert list(knn["mae"]) == list(knn["subject_mae"]) == [1, 3] and list(lin["mae"]) == list(lin["subject_mae"]) == list(probe.l2)
        for out, variants in ((knn, [(k, knn["predictions"][k]) for k in (1, 3)]), (lin, [(l2, lin["predictions"][h]) for h, l2 in enumerate(probe.l2)])):
            for key, pred in variants:
                pred = pred.cpu().double()
                assert pred.shape == (7, 2) and not torch.isnan(pred).any()
                close(out["mae"][key], mae64(pred, t64))
                close(out["subject_mae"][key], mae64(subject_means(pred), subject_means(t64)))
                assert math.isnan(out["mae"][key][1]) == math.isnan(out["subject_mae"][key][1]) == empty and not math.isnan(out["mae"][key][0])
    # classification.  Query 0 (subject 0, one volume) IS bank row 0, whose label is -1 (none): at k = 1 its only neighbour casts no vote, so
    # the volume's and the subject's class are -1 and both are misses - although the subject's label is 0, the arg-max of its all-zero scores
    labels = torch.tensor([-1, 0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 1])
    y = torch.tensor([0, 0, 1, 1, 0, 1, 0])
    Qc = X[[0, 1, 4, 2, 3, 5, 6]] + torch.cat([torch.zeros(1, 8), 0.01 * torch.randn(6, 8, generator=torch.Generator().manual_seed(35))]).cuda()
    cbank = FeatureBank.from_features(X, labels=labels, groups=torch.arange(12) + 3)
    knn = knn_evaluate(cbank, Qc, labels=y, k=(1, 3), query_groups=GROUPS, num_classes=2)
    assert int(knn["predictions"][1][0]) == -1 and knn["scores"][1][0].tolist() == [0.0, 0.0] and int(knn["predictions"][3][0]) >= 0
    y_subject = torch.tensor([0, 0, 1])                          # the label of each subject's first volume
    for k in (1, 3):
        pooled = subject_means(knn["scores"][k].cpu().double())
        best, cls = pooled.max(dim=1)
        assert all(abs(float(a - b)) > 1e-6 for a, b in pooled[1:])                           # no arg-max hangs on the last digits
        cls = torch.where(best > 0, cls, torch.full_like(cls, -1))
        assert (int(cls[0]) == -1) == (k == 1)
        assert knn["acc"][k] == pytest.approx((knn["predictions"][k].cpu() == y).double().mean().item(), abs=1e-6)
        assert knn["subject_acc"][k] == pytest.approx((cls == y_subject).double().mean().item(), abs=1e-6)
    # k = 1: the neighbours of the other queries are the rows they were made from - subject 1 votes [1, 0], subject 2 [0.25, 0.75]: both hits
    assert knn["subject_acc"][1] == pytest.approx(2 / 3, abs=1e-6) and knn["acc"][1] == pytest.approx(4 / 7, abs=1e-6)
    cprobe = LinearProbe(8, num_classes=2, l2=[1e-3, 0.1]).fit(cbank, steps=20)
    lin = linear_evaluate(cprobe, Qc, labels=y, query_groups=GROUPS)
    assert list(lin["acc"]) == list(lin["subject_acc"]) == list(cprobe.l2)
    for h, l2 in enumerate(cprobe.l2):
        pooled = subject_means(lin["probs"][h].cpu().double())
        assert (pooled[:, 0] - pooled[:, 1]).abs().min() > 1e-6   # no arg-max hangs on the last digits
        assert lin["acc"][l2] == pytest.approx((lin["predictions"][h].cpu() == y).double().mean().item(), abs=1e-6)
        assert lin["subject_acc"][l2] == pytest.approx((pooled.argmax(dim=1) == y_subject).double().mean().item(), abs=1e-6)      # plain arg-max
