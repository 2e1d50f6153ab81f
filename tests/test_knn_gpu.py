"""Frozen-feature evaluation on the MI355X: nv_knn_topk, nv_knn_vote, nv_pool_features and nv_segment_mean held to the float64 restatement
(tests/knn_ref.py; what it is worth is proven in tests/test_knn_cpu.py), then the model level: ViT.forward_features /
NeuroEncoder.extract_features, features.FeatureBank / knn_predict / knn_evaluate and the Trainer's kNN validation.

Measured on one MI355X (gfx950): the integer cases bit-equal at 1, 2, 3, 7 and automatic splits; unit-norm inputs: worst |sim - float64| over
the bound d 2^-24 sum |a||b| 0.059 (d = 72) and 0.017 (d = 768), largest absolute error 7.7e-7; softmax vote against float64 3.7e-8 (scores)
and 3.0e-8 (regression) relative, gate 1e-5."""
import numpy as np
import pytest
import torch

import knn_ref as R
import ld_windows as L
import weights as W
from conftest import rel_err, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import ops
    return ops


def dev(t, dtype=None):
    if t is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return (t if dtype is None else t.to(dtype)).cuda()


def bits_equal(a, b):
    """two float32 / int32 arrays word for word (numpy on the host)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ------------------------------------------------------------------ 1. integer inputs, exact
@pytest.mark.parametrize("case", R.INT_CASES, ids=lambda c: "d%d-q%d-b%d-k%d-%s-pad%d" % c)
def test_topk_integer_inputs_bit_equal_at_every_split(ops, case):
    d, Nq, Nb, k, groups, pad = case
    Q, bank, qg, bg = R.int_case(d, Nq, Nb, k, groups, seed=Nq * 1000 + Nb)
    want_idx, want_sim = R.topk_ref(R.sims_f64(Q, bank), k, qg, bg)
    # padded leading dimensions with NaN guard columns and rows: a guard cell that reaches a dot product shows up in sim
    Qd = L.into_poisoned(torch.from_numpy(Q), pad) if pad else dev(Q)
    Bd = L.into_poisoned(torch.from_numpy(bank), pad) if pad else dev(bank)
    assert Qd.stride(0) == d + pad and Bd.stride(0) == d + pad
    for splits in R.INT_SPLITS:
        idx, sim = ops.knn_topk(Qd, Bd, k, dev(qg), dev(bg), splits=splits)
        assert bits_equal(idx.cpu().numpy(), want_idx), (case, splits)
        assert bits_equal(sim.cpu().numpy(), want_sim), (case, splits)
    idx, sim = ops.knn_topk(Qd, Bd, k, dev(qg), dev(bg))                       # the automatic split count
    assert bits_equal(idx.cpu().numpy(), want_idx) and bits_equal(sim.cpu().numpy(), want_sim)
    if groups == "all":
        assert (want_idx[0] == -1).all() and np.isneginf(want_sim[0]).all()      # nothing eligible: every slot empty
    if Nb < k:
        assert (want_idx[:, Nb:] == -1).all()


# ------------------------------------------------------------------ 2. random unit-norm inputs
@pytest.mark.parametrize("d,Nq,Nb,k", [(72, 67, 1000, 20), (768, 130, 1000, 20), (768, 5, 200, 128)])
def test_topk_unit_norm_inputs_within_the_fp32_bound_and_split_independent(ops, d, Nq, Nb, k):
    Q, bank = R.unit_case(d, Nq, Nb, seed=d + Nq)
    sims, bound = R.sims_f64(Q, bank), R.dot_bound(Q, bank, d)
    Qd, Bd = dev(Q), dev(bank)
    first = None
    for splits in (1, 2, 3, 7, 0, 1):                                          # the forced counts, the automatic one, and the first again (a second run)
        idx, sim = ops.knn_topk(Qd, Bd, k, splits=splits)
        got = (idx.cpu().numpy(), sim.cpu().numpy())
        if first is None:
            first = got
        assert bits_equal(got[0], first[0]) and bits_equal(got[1], first[1]), splits
    idx, sim = first
    assert (idx >= 0).all() and (idx < Nb).all()
    rows = np.arange(Nq)[:, None]
    err = np.abs(sim.astype(np.float64) - sims[rows, idx])
    worst = (err / bound[rows, idx]).max()
    print(f"knn_topk d={d} Nq={Nq} Nb={Nb} k={k}: worst |sim - f64| / bound = {worst:.3f}, largest abs error {err.max():.2e}")
    report(f"knn_topk unit-norm d={d} Nq={Nq} Nb={Nb} k={k}: worst |sim - f64| / (d 2^-24 sum|a||b|) = {worst:.3f}, abs {err.max():.2e}")
    assert (err <= bound[rows, idx]).all()
    # sorted under the order rule: sim descending, equal sim by ascending index; no index twice
    assert ((sim[:, :-1] > sim[:, 1:]) | ((sim[:, :-1] == sim[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))).all()
    assert all(len(set(r)) == k for r in idx)
    # nothing returned lies more than two bounds below the true k-th similarity
    kth = -np.sort(-sims, axis=1)[:, k - 1]
    assert (sim.astype(np.float64) >= kth[:, None] - 2 * bound.max(1)[:, None]).all()


# ------------------------------------------------------------------ 3. vote
VOTE = dict(Nq=24, Nb=40, kmax=20, C=5, K=3, seed=11)          # the case tests/test_knn_cpu.py proves the margins of


def test_vote_uniform_bit_equal_softmax_within_the_gate(ops):
    idx, sim, labels, targets = R.vote_case(**VOTE)
    di, ds, dl, dt = dev(idx), dev(sim), dev(labels), dev(targets)
    C, worst_c, worst_r = VOTE["C"], 0.0, 0.0
    for k in (20, 10, 5):
        want_sc, want_pred, _ = R.vote_cls_ref(idx, sim, k, "uniform", 0.07, labels, C)
        sc, pred = ops.knn_vote(di, ds, k, labels=dl, num_classes=C, weights="uniform")
        assert bits_equal(sc.cpu().numpy(), want_sc) and np.array_equal(pred.cpu().numpy(), want_pred)
        assert pred[0].item() == 1 and pred[1].item() == -1 and (sc[1] == 0).all().item()          # the tied vote goes to the lower class; the empty row
        want_r, _ = R.vote_reg_ref(idx, sim, k, "uniform", 0.07, targets)
        pr = ops.knn_vote(di, ds, k, targets=dt, weights="uniform").cpu().numpy()
        assert bits_equal(pr, want_r) and np.isnan(pr[1]).all() and np.isnan(pr[3]).all()              # NaN words included: one quiet NaN pattern
        # softmax weights: fp32 expf of an fp32 argument against float64
        _, want_pred, want64 = R.vote_cls_ref(idx, sim, k, "softmax", 0.07, labels, C)
        sc, pred = ops.knn_vote(di, ds, k, labels=dl, num_classes=C, weights="softmax", temperature=0.07)
        worst_c = max(worst_c, rel_err(sc, want64))
        assert np.array_equal(pred.cpu().numpy(), want_pred)                                       # the gaps are above the gate (CPU test)
        _, want64 = R.vote_reg_ref(idx, sim, k, "softmax", 0.07, targets)
        pr = ops.knn_vote(di, ds, k, targets=dt, weights="softmax", temperature=0.07).cpu().double().numpy()
        assert np.array_equal(np.isnan(pr), np.isnan(want64))
        live = ~np.isnan(want64)
        worst_r = max(worst_r, rel_err(pr[live], want64[live]))
    print(f"knn_vote softmax: scores rel {worst_c:.2e}, regression rel {worst_r:.2e}")
    report(f"knn_vote softmax weights vs float64: scores rel {worst_c:.2e}, regression rel {worst_r:.2e} (gate {R.SOFTMAX_GATE:.0e})")
    assert worst_c < R.SOFTMAX_GATE and worst_r < R.SOFTMAX_GATE


# ------------------------------------------------------------------ 4. pooling and segment mean
@pytest.mark.parametrize("n,d", [(n, d) for n in (2, 9, 28) for d in (8, 72)])
def test_pool_features_bit_equal_in_every_mode(ops, n, d):
    B = 3
    x = np.random.default_rng(n * 100 + d).standard_normal((B, n + 1, d + 4)).astype(np.float32)
    x[1] = 0.0                                                                # a zero sample
    xd = dev(x)[:, :n, :d]                                                    # a strided view: batch stride (n + 1)(d + 4), row stride d + 4
    tok = x[:, :n, :d]
    for mode in (0, 1, 2):
        for normalize in (False, True):
            want = R.pool_ref(tok, mode, normalize)
            got = ops.pool_features(xd, mode, normalize)
            assert bits_equal(got.cpu().numpy(), want), (mode, normalize)
            # row0 > 0 into a bank with guard rows and columns
            bank, buf = L.padded(B + 2, d, torch.float32, pad_cols=4)
            ops.pool_features(xd, mode, normalize, out=bank, row0=2)
            assert bits_equal(bank[2:].cpu().numpy(), want)
            keep = buf.clone()
            top = (bank.data_ptr() - buf.data_ptr()) // buf.stride(0)
            keep[top + 2:top + 2 + B, :4 * d] = L.SENTINEL
            assert bool((keep == L.SENTINEL).all()), (mode, normalize)          # rows 0, 1 of the bank and every guard cell untouched
    from neurovit_amd._cabi import lib
    tm = torch.empty((B, d), device="cuda")
    dense = dev(tok)
    assert lib.nv_token_mean(dense.data_ptr(), B, n, d, tm.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert torch.equal(tm, ops.pool_features(dense, "mean"))                   # the bits of nv_token_mean


@pytest.mark.parametrize("w", [5, 72, 300])
def test_segment_mean_bit_equal(ops, w):
    rng = np.random.default_rng(w)
    N, G = 23, 6
    src = rng.standard_normal((N, w + 4)).astype(np.float32)
    groups = rng.integers(0, G, size=N)
    groups[groups == 4] = 2                                                   # segment 4 is empty
    groups[5] = -1                                                            # a row in no segment
    order, offsets = R.csr_of(groups, G)
    o2, f2 = ops.segment_csr(groups, G)
    assert np.array_equal(o2.cpu().numpy()[:offsets[-1]], order[:offsets[-1]]) and np.array_equal(f2.cpu().numpy(), offsets)
    order[offsets[0]:offsets[1]] = order[offsets[0]:offsets[1]][::-1]       # an unsorted order: the sum follows it
    rng.shuffle(order[offsets[2]:offsets[3]])
    want = R.segment_mean_ref(src[:, :w], order, offsets)
    sd = dev(src)[:, :w]
    out, buf = L.padded(G, w, torch.float32, pad_cols=4)
    ops.segment_mean(sd, dev(order), dev(offsets), out=out)
    assert bits_equal(out.cpu().numpy(), want) and L.guards_intact(out, buf)
    assert (out[4] == 0).all().item()


# ------------------------------------------------------------------ 5. model level, on the micro config
def micro_vit(pool, seed=1):
    from neurovit_amd.vit_3d import ViT
    model = ViT(**dict(W.MICRO, pool=pool)).cuda()
    model.load_state_dict(W.make_tensors(W.vit_param_spec(**W.MICRO), seed), strict=True)
    return model


def micro_video(B, seed):
    S = W.MICRO["image_size"]
    return W.make_volume((B, S, S, S), seed).cuda().unsqueeze(1)              # [B, C = 1, F, H, W]


@pytest.mark.parametrize("pool", ["cls", "mean"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_own_pooling_feeds_the_head_bit_for_bit(ops, pool, precision):
    model, x = micro_vit(pool), micro_video(3, 5)
    model.train()                                                             # forward_features runs the eval forward whatever the mode
    head = model.mlp_head
    with model.precision(precision):
        feats = model.forward_features(x)
        assert feats.shape == (3, W.MICRO["dim"]) and feats.dtype == torch.float32 and not feats.requires_grad and feats.grad_fn is None
        assert all(p.grad is None for p in model.parameters())                # no graph, no .grad - on a trainable model
        model.eval()
        with torch.no_grad():
            want = model(x)
        logits = ops.head_fwd(feats.view(3, 1, -1), head[0].weight, head[0].bias, head[1].weight, head[1].bias, head[0].eps)[0]
        assert torch.equal(logits, want), (pool, precision)
        # every pooling against nv_pool_features on the tokens of an eval forward (rows_form = 1 where the pooling reads every row)
        for name in ("cls", "mean", "patch_mean"):
            for normalize in (False, True):
                got = model.forward_features(x, pool=name, normalize=normalize).clone()
                form = None if name == "cls" else 1                            # the cls row alone comes from the forward's default form (forward()'s own)
                if precision == "fp32":
                    model._rt.forward_f32(x, model._arena, rows_form=form)
                else:
                    model._refresh_shadow()
                    model._rt.forward_lnfold(x, model._arena, model._shadow, model._fresh_fold(), rows_form=form)
                tokens = model._last_tokens()
                assert torch.equal(got, ops.pool_features(tokens, name, normalize)), (name, normalize)
                if name == "patch_mean" and not normalize:
                    assert bits_equal(got.cpu().numpy(), R.pool_ref(tokens.cpu().numpy(), 2))
                    assert rel_err(got, tokens[:, 1:].double().mean(1)) < 1e-6
                if normalize:
                    assert rel_err(got.double().norm(dim=1), torch.ones(3)) < 1e-6
        # a frozen model; out / row0 fill a bank in place
        for p in model.parameters():
            p.requires_grad_(False)
        bank = torch.full((5, W.MICRO["dim"]), 7.0, device="cuda")
        rows = model.forward_features(x, out=bank, row0=2)
        assert rows.data_ptr() == bank[2:].data_ptr() and torch.equal(bank[2:], feats) and (bank[:2] == 7.0).all().item()


def test_refusals_raise_what_the_docs_say(ops):
    model, x = micro_vit("cls"), micro_video(2, 6)
    with pytest.raises(NotImplementedError, match="fused 4D input form"):
        model.forward_features(x, time_points=4)
    with pytest.raises(ValueError, match="pool must be"):
        model.forward_features(x, pool="max")
    with pytest.raises(ValueError, match="expected video"):
        model.forward_features(x[:, :, :8])
    handle = model.transformer.layers[0][0].attend.register_forward_hook(lambda m, i, o: None)
    with pytest.raises(NotImplementedError, match="per-head maps"):
        model.forward_features(x)
    handle.remove()
    model.eval()
    model.enable_fp8(x)
    with pytest.raises(NotImplementedError, match="fp8"):
        model.forward_features(x)
    with model.precision("fp32"):
        assert model.forward_features(x).shape == (2, W.MICRO["dim"])           # the fp32 forward reads no e4m3 operand
    model.disable_fp8()
    with pytest.raises(ValueError, match="together"):
        ops.knn_topk(torch.zeros(4, 8, device="cuda"), torch.zeros(4, 8, device="cuda"), 2, torch.zeros(4, dtype=torch.int32, device="cuda"), None)


SIZE = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=2, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=128)


def test_bank_predict_and_evaluate_equal_the_composition_of_the_ops(ops):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd import FeatureBank, knn_evaluate, knn_predict
    torch.manual_seed(3)
    model = ne.NeuroEncoder(W.neuro_config(12, 3, DEVICE="cuda:0", **SIZE))
    vols = [W.make_volume((4, 12, 12, 12), 40 + i).cuda() for i in range(3)]
    labels = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2])
    subjects = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5])
    bank = FeatureBank(64, 12)
    for i, v in enumerate(vols):
        bank.append(model, v, labels[4 * i:4 * i + 4], subjects[4 * i:4 * i + 4], pool="patch_mean")
    assert bank.size == 12
    want = torch.cat([model.extract_features(v, pool="patch_mean", normalize=True).clone() for v in vols])
    assert torch.equal(bank.view(), want)
    assert torch.equal(model.extract_features(vols[0]), model.volume_encoder.vit3d.forward_features(vols[0].permute(0, 3, 1, 2).unsqueeze(1)))
    # a bank queried with itself under groups = arange never returns the query row; under its subjects never a row of the query's subject
    own = FeatureBank.from_features(bank.view(), labels=labels, groups=torch.arange(12))
    _, _, idx, sim = knn_predict(own, own.view(), k=5, query_groups=torch.arange(12), num_classes=3)
    assert (idx != torch.arange(12, device="cuda", dtype=torch.int32)[:, None]).all().item() and (idx >= 0).all().item()
    _, _, idx, _ = knn_predict(bank, bank.view(), k=12, query_groups=subjects, num_classes=3)
    sub = subjects.cuda()
    assert ((idx < 0) | (sub[idx.clamp(min=0).long()] != sub[:, None])).all().item() and (idx[:, 10:] == -1).all().item() and (idx[:, :10] >= 0).all().item()
    _, _, idx0, _ = knn_predict(bank, bank.view(), k=1, num_classes=3)
    assert torch.equal(idx0[:, 0], torch.arange(12, device="cuda", dtype=torch.int32))          # without groups a unit row's nearest neighbour is itself
    # knn_evaluate = the ops, composed
    q = bank.view()[[1, 4, 7, 10, 2, 5]].contiguous()
    ql, qs = labels[[1, 4, 7, 10, 2, 5]], subjects[[1, 4, 7, 10, 2, 5]]
    got = knn_evaluate(bank, q, labels=ql, k=(3, 5), temperature=0.07, query_groups=qs, num_classes=3)
    i2, s2 = ops.knn_topk(q, bank.view(), 5, qs.to(torch.int32).cuda(), bank.groups[:12])
    assert torch.equal(got["idx"], i2) and torch.equal(got["sim"], s2)
    order, offsets = ops.segment_csr(qs)
    for k in (3, 5):
        sc, pr = ops.knn_vote(i2, s2, k, labels=bank.labels[:12], num_classes=3, weights="softmax", temperature=0.07)
        assert torch.equal(got["scores"][k], sc) and torch.equal(got["predictions"][k], pr)
        assert got["acc"][k] == (pr == ql.to(torch.int32).cuda()).float().mean().item()
        pooled = ops.segment_mean(sc, order, offsets).cpu()
        filled = (offsets[1:] > offsets[:-1]).cpu()
        first = {int(s): int(l) for s, l in reversed(list(zip(qs.tolist(), ql.tolist())))}
        hits = sum(int(filled[g]) and int(pooled[g].argmax()) == first[g] for g in range(len(filled)) if int(filled[g]))
        assert got["subject_acc"][k] == pytest.approx(hits / int(filled.sum()), abs=1e-7)
    # the subject-level bank and a regression vote
    by = bank.by_group()
    assert by.size == 6 and torch.equal(by.labels[:6].cpu(), labels[::2].to(torch.int32))
    assert rel_err(by.view().double().norm(dim=1), torch.ones(6)) < 1e-6
    raw = ops.segment_mean(bank.view(), *ops.segment_csr(subjects))
    assert torch.equal(by.view(), ops.pool_features(raw.view(6, 1, 64), "cls", True))
    targets = torch.arange(24, dtype=torch.float32).reshape(12, 2)
    targets[3, 1] = float("nan")
    reg = FeatureBank.from_features(bank.view(), targets=targets, groups=subjects)
    out = knn_evaluate(reg, q, targets=targets[[1, 4, 7, 10, 2, 5]], k=5, weights="uniform", query_groups=qs)
    pr = ops.knn_vote(i2, s2, 5, targets=reg.targets[:12], weights="uniform")
    assert torch.equal(out["predictions"][5], pr)
    m = ops.RegressionMetrics(2)
    m.update(pr, targets[[1, 4, 7, 10, 2, 5]].cuda())
    assert out["mae"][5] == m.compute()["mae"].tolist() and len(out["subject_mae"][5]) == 2


def test_subject_label_of_the_score_with_empty_unassigned_and_mixed_subjects(ops):
    """knn_evaluate takes a subject's label from ops.Segments.labels (nv_segment_labels).  Held to the gather it replaced - the label of the
    subject's first row, the subjects without a row masked - on ids that use every branch: subject 3 of the 6 has no query, two queries
    belong to no subject (-1), subject 2 carries two labels."""
    from neurovit_amd.features import FeatureBank, knn_evaluate
    Nq, Nb, d, k, G, C = 40, 64, 16, 5, 6, 3
    gen = torch.Generator().manual_seed(55)
    centres = 2.0 * torch.randn(C, d, generator=gen)
    bl, ql = torch.arange(Nb) % C, torch.arange(Nq) % C
    bank = FeatureBank.from_features((centres[bl] + torch.randn(Nb, d, generator=gen)).cuda(), labels=bl, groups=torch.arange(Nb) % G)
    q = (centres[ql] + 1.5 * torch.randn(Nq, d, generator=gen)).cuda()
    qs = torch.tensor([0, 1, 2, 4, 5])[torch.arange(Nq) % 5]
    qs[7], qs[23] = -1, -1
    ql[qs == 0], ql[qs == 1], ql[qs == 4], ql[qs == 5] = 0, 1, 2, 0          # one label per subject ...
    ql[qs == 2] = torch.tensor([1, 1, 2, 1, 1, 1, 1])                         # ... but for subject 2, whose third row differs from its first
    got = knn_evaluate(bank, q, labels=ql, k=k, query_groups=qs, num_classes=C)
    order, offsets = ops.segment_csr(qs)
    assert offsets.numel() - 1 == G
    filled = offsets[1:] > offsets[:-1]
    assert filled.tolist() == [True, True, True, False, True, True]
    y = ql.to(torch.int32).cuda()
    y_subject = y[order[offsets[:-1].clamp(max=Nq - 1).long()].long()]
    best, cls = ops.segment_mean(got["scores"][k], order, offsets).max(dim=1)
    cls = torch.where(best > 0, cls.to(torch.int32), torch.full_like(cls, -1, dtype=torch.int32))
    want = (((cls == y_subject) & filled).float().sum() / filled.float().sum().clamp(min=1)).item()
    print(f"subject label: subject_acc {got['subject_acc'][k]!r}, by the gather {want!r}, acc {got['acc'][k]!r}")
    assert got["subject_acc"][k] == want and 0.0 < want <= 1.0
    assert int(cls[3]) == -1 and int(y_subject[3]) != -1                      # the empty subject: no class, a label from the clamped gather - masked, not a hit
    metrics = ops.ClassificationMetrics(C, capacity=Nq)
    metrics.update(got["scores"][k], ql, groups=qs, kind="probs")
    assert metrics.compute()["subject_mixed_labels"] == 1


def test_trainer_logs_the_knn_validation_only_when_asked(tmp_path, monkeypatch):
    import neurovit_amd.NeuroEncoder as ne
    from neurovit_amd.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    vols = torch.cat([(W.make_volume((3, 12, 12, 12), 83 + i) * 1.5) for i in range(2)])
    names = torch.tensor([0, 0, 1, 1, 2, 2])
    labels = torch.tensor([0, 1, 0, 1, 0, 1])
    ds = torch.utils.data.TensorDataset(names, torch.zeros(6, 1), vols, labels)
    base = dict(W.neuro_config(12, 3, DEVICE="cuda:0", **SIZE), GLOBAL_OUTPUT_DIR=str(tmp_path / "out"), TRAINING_EPOCHS=2, TRAINING_BATCH_SIZE=3,
                TRAINING_NUM_WORKERS=0, TRAINING_OBJECTIVE="mim", PRETRAIN_MASK_RATIO=0.5, TRAINING_LEARNING_RATE=1e-3)

    def logged(cfg):
        torch.manual_seed(84)
        trainer = Trainer(cfg, ne.NeuroEncoder(cfg), ds, ds)
        seen = []
        trainer._log = seen.append
        for epoch in range(2):
            trainer.train(epoch)
            trainer.validate(epoch)
        return trainer, seen

    plain_trainer, plain = logged(base)
    assert plain_trainer.knn is None and Trainer.knn_from_config(dict(base, PRETRAIN_KNN_EVERY=0)) is None
    assert all(set(p) <= {"epoch", "batch", "recon_loss", "learning_rate", "duration", "val_recon_loss"} for p in plain)       # what it logged before: nothing of the kNN
    assert [p for p in plain if "val_recon_loss" in p] and not any("val_knn_acc" in p for p in plain)
    trainer, with_knn = logged(dict(base, PRETRAIN_KNN_EVERY=2, PRETRAIN_KNN_K=[1, 3], PRETRAIN_KNN_TEMPERATURE=0.1))
    drop_time = lambda ps: [{k: v for k, v in p.items() if k != "duration"} for p in ps]
    extra = [p for p in with_knn if "val_knn_acc" in p]
    assert drop_time([p for p in with_knn if "val_knn_acc" not in p]) == drop_time(plain)                                  # the same training, the same records
    assert len(extra) == 1 and set(extra[0]) == {"epoch", "val_knn_acc", "val_knn_subject_acc", "val_knn_acc_k3", "val_knn_subject_acc_k3"} and extra[0]["epoch"] == 1
    assert all(0.0 <= extra[0][k] <= 1.0 for k in extra[0] if k != "epoch")
    trainer.model.train()
    on_demand = trainer.knn_validate()
    assert trainer.model.training                                                                                         # the mode it was found in
    assert {k: v for k, v in extra[0].items() if k != "epoch"} == on_demand                                                # reproducible: the same bits, the same figures
    with pytest.raises(ValueError, match="PRETRAIN_KNN_K"):
        Trainer.knn_from_config(dict(base, PRETRAIN_KNN_EVERY=1, PRETRAIN_KNN_K=129))
