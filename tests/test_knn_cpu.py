"""What tests/knn_ref.py (the restatement tests/test_knn_gpu.py holds the frozen-feature kernels to) is worth, proven without a GPU: top-k
against a brute-force sort and torch.topk, the vote against direct float64 formulas, pooling against F.normalize in double, the segment
mean against a per-group loop; planted defects must fail; the properties the GPU tests rely on (ties across the k-th place, score gaps above
the softmax gate) hold on the very inputs they use.  Plus the header / binding side of the new entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_topk(sims, k, qg=None, bg=None):
    Nq, Nb = sims.shape
    idx = np.full((Nq, k), -1, np.int32)
    out = np.full((Nq, k), -np.inf, np.float32)
    for q in range(Nq):
        elig = [j for j in range(Nb) if not (qg is not None and qg[q] >= 0 and qg[q] == bg[j])]
        best = sorted(elig, key=lambda j: (-sims[q, j], j))[:k]
        idx[q, :len(best)] = best
        out[q, :len(best)] = sims[q, best]
    return idx, out


CPU_CASES = [c for c in R.INT_CASES if c[1] * c[2] <= 20000]


@pytest.mark.parametrize("case", R.INT_CASES, ids=lambda c: "d%d-q%d-b%d-k%d-%s" % c[:5])
def test_integer_cases_are_exact_in_fp32_and_tie_across_the_kth_place(case):
    d, Nq, Nb, k, groups, _ = case
    Q, bank, qg, bg = R.int_case(d, Nq, Nb, k, groups, seed=Nq * 1000 + Nb)
    assert np.abs(Q).max() <= 8 and np.abs(bank).max() <= 8 and d <= 72 and (Q == np.round(Q)).all() and (bank == np.round(bank)).all()
    sims = R.sims_f64(Q, bank)
    assert np.abs(sims).max() < 2 ** 24 and (sims.astype(np.float32) == sims).all()          # every partial sum is an integer below 2^24
    if Nb > k:
        frac = R.kth_place_ties(sims, k, qg, bg)
        assert frac >= 0.5, f"only {frac:.2f} of the queries tie across the k-th place"      # the coverage condition of the integer case
    if groups == "all":
        idx, _ = R.topk_ref(sims[:1], k, qg[:1], bg)
        assert (idx == -1).all()                                                            # a query with nothing eligible


@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: "d%d-q%d-b%d-k%d-%s" % c[:5])
def test_topk_restatement_against_a_brute_force_sort(case):
    d, Nq, Nb, k, groups, _ = case
    Q, bank, qg, bg = R.int_case(d, Nq, Nb, k, groups, seed=Nq * 1000 + Nb)
    sims = R.sims_f64(Q, bank)
    idx, sim = R.topk_ref(sims, k, qg, bg)
    want_idx, want_sim = brute_topk(sims, k, qg, bg)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    if Nb < k or groups != "none":
        assert ((idx == -1) == np.isneginf(sim)).all()


def test_topk_restatement_against_torch_topk_without_ties():
    Q, bank = R.unit_case(72, 37, 300, seed=1)
    sims = R.sims_f64(Q, bank)
    assert all(len(np.unique(r)) == len(r) for r in sims)
    idx, sim = R.topk_ref(sims, 20)
    v, i = torch.from_numpy(sims).topk(20, dim=1)
    assert np.array_equal(idx, i.numpy().astype(np.int32)) and np.array_equal(sim, v.numpy().astype(np.float32))
    assert np.array_equal(idx, brute_topk(sims, 20)[0])


def test_planted_topk_defects_fail():
    d, Nq, Nb, k, groups = 8, 67, 63, 5, "some"
    Q, bank, qg, bg = R.int_case(d, Nq, Nb, k, groups, seed=5)
    sims = R.sims_f64(Q, bank)
    good = R.topk_ref(sims, k, qg, bg)[0]
    assert np.array_equal(good, brute_topk(sims, k, qg, bg)[0])
    assert not np.array_equal(R.topk_ref(sims, k, qg, bg, tie_high=True)[0], good)                    # ties to the higher index
    qneg, bneg = qg.copy(), bg.copy()
    bneg[::4] = -1                                                                                    # bank rows of no group; queries of no group must still see them
    good = R.topk_ref(sims, k, qneg, bneg)[0]
    assert np.array_equal(good, brute_topk(sims, k, qneg, bneg)[0]) and (qneg < 0).any()
    assert not np.array_equal(R.topk_ref(sims, k, qneg, bneg, ignore_negative_group=True)[0], good)   # a group test that ignores q_group < 0


VOTE = dict(Nq=24, Nb=40, kmax=20, C=5, K=3, seed=11)


def direct_softmax_vote(idx, sim, k, T, labels, C):
    scores = np.zeros((idx.shape[0], C))
    for q in range(idx.shape[0]):
        use = [i for i in range(k) if idx[q, i] >= 0]
        if not use:
            continue
        s = np.array([sim[q, i] for i in use], np.float64) / np.float64(np.float32(T))
        w = np.exp(s - s.max())
        w /= w.sum()                                       # softmax(sim / T): exp(sim / T) up to the common factor
        for wi, i in zip(w, use):
            scores[q, labels[idx[q, i]]] += wi
    return scores


def test_vote_restatement_against_direct_float64_votes():
    idx, sim, labels, targets = R.vote_case(**VOTE)
    for k in (20, 10, 5):
        sc32, pred, sc = R.vote_cls_ref(idx, sim, k, "softmax", 0.07, labels, VOTE["C"])
        want = direct_softmax_vote(idx, sim, k, 0.07, labels, VOTE["C"])
        assert np.abs(sc - want).max() < 1e-12
        assert np.array_equal(pred, np.where(want.sum(1) > 0, want.argmax(1), -1))
        top2 = -np.sort(-sc, axis=1)[:, :2]
        live = sc.sum(1) > 0
        assert (top2[live, 0] - top2[live, 1] > 10 * R.SOFTMAX_GATE).all()       # what the GPU test's softmax predictions rely on
        # uniform: counts
        sc32, pred, sc = R.vote_cls_ref(idx, sim, k, "uniform", 0.07, labels, VOTE["C"])
        for q in range(VOTE["Nq"]):
            labs = [labels[j] for j in idx[q, :k] if j >= 0]
            cnt = np.bincount(labs, minlength=VOTE["C"]) if labs else np.zeros(VOTE["C"])
            assert np.array_equal(sc[q], cnt / max(len(labs), 1))
            assert pred[q] == (cnt.argmax() if labs else -1)                     # np.argmax: ties to the lower class
        assert pred[0] == 1 and (k % 2 or sc[0, 1] == sc[0, 2] == 0.5)            # the planted tied vote (every even prefix)
        assert pred[1] == -1 and (sc[1] == 0).all()                               # the empty row
        # regression
        p32, p = R.vote_reg_ref(idx, sim, k, "softmax", 0.07, targets)
        for q in range(VOTE["Nq"]):
            for c in range(VOTE["K"]):
                use = [i for i in range(k) if idx[q, i] >= 0 and not np.isnan(targets[idx[q, i], c])]
                if not use:
                    assert np.isnan(p[q, c])
                    continue
                w = np.exp((sim[q, use].astype(np.float64) - np.float64(sim[q, 0])) / np.float64(np.float32(0.07)))
                assert abs(p[q, c] - (w * targets[idx[q, use], c]).sum() / w.sum()) < 1e-12
        assert np.isnan(p[1]).all() and np.isnan(p[3]).all()                      # no neighbour; one neighbour with nothing observed


def test_planted_vote_defect_fails():
    idx, sim, labels, _ = R.vote_case(**VOTE)
    good = R.vote_cls_ref(idx, sim, 20, "uniform", 0.07, labels, VOTE["C"])
    bad = R.vote_cls_ref(idx, sim, 20, "uniform", 0.07, labels, VOTE["C"], count_empty=True)      # -1 slots counted in the vote
    assert not np.array_equal(good[0], bad[0]) and bad[1][1] != -1


POOL_SHAPES = [(n, d) for n in (2, 9, 28) for d in (8, 72)]


def pool_tokens(B, n, d, seed):
    x = np.random.default_rng(seed).standard_normal((B, n, d)).astype(np.float32)
    x[1] = 0.0                                                                     # a zero sample: the 1e-12 floor of the normalisation
    return x


@pytest.mark.parametrize("n,d", POOL_SHAPES)
def test_pool_restatement_against_torch(n, d):
    x = pool_tokens(3, n, d, n * 100 + d)
    t = torch.from_numpy(x)
    assert np.array_equal(R.pool_ref(x, 0), x[:, 0])
    assert np.abs(R.pool_ref(x, 1) - t.double().mean(1).numpy()).max() < 4 * 2.0 ** -24 * n * np.abs(x).max()
    pm = t[:, 1:].double().mean(1)
    assert np.array_equal(R.pool_ref(x, 2), pm.float().numpy()) or np.abs(R.pool_ref(x, 2) - pm.numpy()).max() < 2.0 ** -24 * np.abs(x).max()
    for mode in (0, 1, 2):
        pooled = torch.from_numpy(R.pool_ref(x, mode))
        want = F.normalize(pooled.double(), dim=1).numpy()
        got = R.pool_ref(x, mode, normalize=True)
        assert np.abs(got - want).max() <= 2.0 ** -24                            # one rounding of values in [-1, 1] (the sums differ in their last double bit at most)
        assert (got[1] == 0).all() and not np.isnan(got).any()


def test_segment_mean_restatement_and_csr():
    rng = np.random.default_rng(3)
    src = rng.standard_normal((23, 9)).astype(np.float32)
    groups = rng.integers(0, 6, size=23)
    groups[groups == 4] = 2                                                        # segment 4 is empty
    groups[5] = -1                                                                 # a row in no segment
    order, offsets = R.csr_of(groups, 6)
    assert offsets[5] == offsets[4] and offsets[-1] == 22
    got = R.segment_mean_ref(src, order, offsets)
    for g in range(6):
        rows = src[groups == g]
        want = rows.astype(np.float64).mean(0) if len(rows) else np.zeros(9)
        assert np.abs(got[g] - want).max() < 2.0 ** -23 * max(1.0, np.abs(src).max())
    assert (got[4] == 0).all()
    # the order of the rows within a segment is the CSR's: an unsorted order is a different (still valid) table
    perm = order.copy()
    perm[offsets[0]:offsets[1]] = perm[offsets[0]:offsets[1]][::-1]
    assert np.abs(R.segment_mean_ref(src, perm, offsets) - got).max() < 2.0 ** -22 * np.abs(src).max()


# ------------------------------------------------------------------ header, binding, host-side checks
NEW_SYMBOLS = ("nv_pool_features", "nv_knn_topk", "nv_knn_topk_splits", "nv_knn_topk_workspace_bytes", "nv_knn_vote", "nv_segment_csr_check", "nv_segment_mean")


def test_entry_points_are_declared_bound_and_listed_in_the_makefile():
    from neurovit_amd import _cabi
    for name in NEW_SYMBOLS:
        assert name in _cabi.lib.protos, name
        assert hasattr(_cabi.lib.load(), name), name
    assert _cabi.lib.protos["nv_knn_topk_workspace_bytes"][0] is ctypes.c_long
    header = open(_cabi.HEADER).read()
    assert re.search(r"#define\s+NV_ABI_VERSION\s+8\b", header) and "#define NV_KNN_MAX_K 128" in header      # new symbols within revision 8
    assert _cabi.POOL_MODES == R.POOL_MODES and _cabi.KNN_MAX_K == 128
    mk = open(os.path.join(ROOT, "neurovit_amd", "csrc", "Makefile")).read()
    assert "features.hip" in mk


def test_host_side_refusals_happen_before_any_launch():
    """bad arguments only: every call returns NV_ERR_ARG from the host-side checks, so this runs without a GPU"""
    from neurovit_amd._cabi import last_error, lib
    buf = (ctypes.c_float * 64)()
    ibuf = (ctypes.c_int * 64)()
    p, ip = ctypes.addressof(buf), ctypes.addressof(ibuf)
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 4, 8, 0, None, None, 0, ip, p, None, 0, None) != 0 and "k=0" in last_error()
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 4, 8, 129, None, None, 0, ip, p, None, 0, None) != 0
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 4, 6, 2, None, None, 0, ip, p, None, 0, None) != 0 and "multiples of 4" in last_error()
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 4, 8, 2, ip, None, 0, ip, p, None, 0, None) != 0 and "together" in last_error()
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 200, 8, 2, None, None, 2, ip, p, None, 0, None) != 0 and "workspace" in last_error()
    assert lib.nv_knn_topk(p, 8, 4, p, 8, 4, 8, 2, None, None, 65, ip, p, None, 0, None) != 0
    assert lib.nv_knn_topk_workspace_bytes(130, 1000, 20, 1) == 0 and lib.nv_knn_topk_workspace_bytes(130, 1000, 20, 3) == 3 * 130 * 20 * 8
    assert lib.nv_knn_topk_splits(8680, 78820, 0) == 8 and lib.nv_knn_topk_splits(1, 3, 0) == 1 and lib.nv_knn_topk_splits(1, 3, 7) == 7
    assert lib.nv_knn_topk_splits(0, 3, 0) == 0
    assert lib.nv_pool_features(p, 16, 8, 1, 1, 8, 2, 0, p, 8, 0, None) != 0 and "n >= 2" in last_error()
    assert lib.nv_pool_features(p, 16, 8, 1, 2, 8, 3, 0, p, 8, 0, None) != 0 and "mode" in last_error()
    assert lib.nv_pool_features(p, 16, 4, 1, 2, 8, 0, 0, p, 8, 0, None) != 0
    assert lib.nv_knn_vote(ip, p, 4, 8, 9, 0, 0.07, 8, ip, 3, p, ip, None, 0, None, None) != 0
    assert lib.nv_knn_vote(ip, p, 4, 8, 8, 1, 0.0, 8, ip, 3, p, ip, None, 0, None, None) != 0 and "temperature" in last_error()
    assert lib.nv_knn_vote(ip, p, 4, 8, 8, 0, 0.07, 8, ip, 3, p, ip, p, 2, p, None) != 0 and "one of the two" in last_error()
    order, offsets = (ctypes.c_int * 4)(0, 1, 2, 3), (ctypes.c_int * 3)(0, 2, 4)
    assert lib.nv_segment_csr_check(order, offsets, 4, 2) == 0
    assert lib.nv_segment_csr_check(order, (ctypes.c_int * 3)(0, 3, 2), 4, 2) != 0 and "decrease" in last_error()
    assert lib.nv_segment_csr_check(order, (ctypes.c_int * 3)(1, 2, 4), 4, 2) != 0
    assert lib.nv_segment_csr_check((ctypes.c_int * 4)(0, 1, 4, 3), offsets, 4, 2) != 0 and "outside" in last_error()
    assert lib.nv_segment_mean(p, 4, 4, 8, ip, ip, 2, p, 8, None) != 0


def test_host_check_program_is_clean_under_the_host_sanitizers():
    """tools/knn_host_check.cpp: the new host entry points (argument checks, workspace sizing, CSR validation) in a stand-alone program built with
    -Xarch_host -fsanitize=address,undefined; it makes bad-argument calls only, so nothing is launched.  Nothing loaded into Python is sanitised."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "neurovit_amd", "csrc"), "host-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "knn_host_check: ok" in out.stdout and "runtime error" not in out.stdout + out.stderr and "AddressSanitizer" not in out.stdout + out.stderr


def test_the_4d_model_refuses_feature_extraction(tmp_path):
    import weights as W
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    size = dict(TRAINING_VIT_DIM=64, TRAINING_VIT_DEPTH=1, TRAINING_VIT_HEADS=1, TRAINING_VIT_MLP_DIM=64)
    model = NeuroEncoder(W.neuro_config(16, 8, **size))
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(16, 8, dim=4, GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **size))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.extract_features(torch.zeros(1, 16, 16, 16))
    with pytest.raises(ValueError, match=r"\[B, H, W, D\]"):
        model.extract_features(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.extract_features(torch.zeros(1, 16, 16, 16))
