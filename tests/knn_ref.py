"""numpy / float64 restatement of the frozen-feature kernels (neurovit_amd/csrc/features.hip): nv_pool_features, nv_knn_topk, nv_knn_vote and
nv_segment_mean, and the inputs the GPU tests run them on.  What the restatement is worth is proven on the CPU in tests/test_knn_cpu.py
(against a brute-force sort, torch.topk, F.normalize and direct float64 votes; planted defects must fail); tests/test_knn_gpu.py holds the
kernels to it.  Where the order of a sum matters it is an explicit ascending loop, not np.sum."""
import numpy as np

POOL_MODES = {"cls": 0, "mean": 1, "patch_mean": 2}
SOFTMAX_GATE = 1e-5          # the project's gate for its loss kernels: fp32 expf of an fp32 argument against float64


# ------------------------------------------------------------------ pooling
def pool_ref(tokens, mode, normalize=False):
    """tokens float32 [B, n, d] -> float32 [B, d].  mode 0 cls row; 1 nv_token_mean's fp32 order; 2 mean of rows 1.. in float64, rounded once."""
    tokens = np.asarray(tokens, np.float32)
    B, n, d = tokens.shape
    out = np.zeros((B, d), np.float32)
    for b in range(B):
        x = tokens[b]
        if mode == 0:
            v = x[0].copy()
        elif mode == 1:
            p = [np.zeros(d, np.float32) for _ in range(4)]
            for g in range(4):
                for t in range(g, n, 4):
                    p[g] = (p[g] + x[t]).astype(np.float32)
            v = (((p[0] + p[1]).astype(np.float32) + (p[2] + p[3]).astype(np.float32)).astype(np.float32) / np.float32(n)).astype(np.float32)
        else:
            s = np.zeros(d, np.float64)
            for t in range(1, n):
                s = s + x[t].astype(np.float64)
            v = (s / np.float64(n - 1)).astype(np.float32)
        if normalize:
            ss = np.float64(0.0)
            for c in range(d):
                ss = ss + np.float64(v[c]) * np.float64(v[c])
            v = (v.astype(np.float64) / max(np.sqrt(ss), 1e-12)).astype(np.float32)
        out[b] = v
    return out


# ------------------------------------------------------------------ top-k
def sims_f64(Q, bank):
    return np.asarray(Q, np.float64) @ np.asarray(bank, np.float64).T


def topk_ref(sims, k, q_group=None, b_group=None, *, tie_high=False, ignore_negative_group=False):
    """sims [Nq, Nb] (any float dtype, compared as given) -> (idx int32 [Nq, k], sim float32 [Nq, k]).  A running best-k list per query, bank rows
    in ascending order: a row enters only if it beats the k-th entry STRICTLY (the entry there has the lower index) and goes behind every
    entry with sim >= its own.  Planted defects for the CPU test: tie_high (equal sim to the higher index), ignore_negative_group (the group
    test forgets q_group >= 0)."""
    sims = np.asarray(sims)
    Nq, Nb = sims.shape
    idx = np.full((Nq, k), -1, np.int32)
    out = np.full((Nq, k), -np.inf, np.float32)
    for q in range(Nq):
        ls, li = [], []
        row = sims[q]
        qg = None if q_group is None or b_group is None else int(q_group[q])
        for j in range(Nb):
            if qg is not None and (qg >= 0 or ignore_negative_group) and qg == int(b_group[j]):
                continue
            s = row[j]
            if len(ls) == k and not (s >= ls[-1] if tie_high else s > ls[-1]):
                continue
            pos = 0
            while pos < len(ls) and (ls[pos] > s if tie_high else ls[pos] >= s):
                pos += 1
            ls.insert(pos, s)
            li.insert(pos, j)
            del ls[k:], li[k:]
        idx[q, :len(li)] = li
        out[q, :len(ls)] = np.asarray(ls, np.float32)
    return idx, out


def kth_place_ties(sims, k, q_group=None, b_group=None):
    """fraction of the queries whose k-th and (k + 1)-th best eligible similarities are equal: the tie rule decides what is returned"""
    hit = 0
    for q in range(sims.shape[0]):
        ok = np.ones(sims.shape[1], bool)
        if q_group is not None and b_group is not None and q_group[q] >= 0:
            ok = np.asarray(b_group) != q_group[q]
        s = np.sort(sims[q][ok])[::-1]
        hit += int(len(s) > k and s[k - 1] == s[k])
    return hit / sims.shape[0]


# the integer cases: (d, Nq, Nb, k, groups, pad) - every d, Nq, Nb and k the kernel's paths turn on appears; each runs at splits 1, 2, 3, 7
INT_SPLITS = (1, 2, 3, 7)
INT_CASES = [
    (8, 1, 3, 1, "none", 0), (8, 5, 3, 5, "some", 4), (20, 5, 63, 5, "none", 4), (20, 67, 64, 20, "some", 0), (72, 67, 65, 20, "none", 8),
    (72, 130, 200, 128, "some", 4), (8, 130, 1000, 20, "all", 4), (20, 1, 1000, 128, "none", 0), (72, 5, 200, 1, "some", 8),
    (8, 67, 63, 128, "all", 0), (20, 130, 65, 5, "none", 4), (72, 1, 64, 20, "some", 4), (72, 67, 1000, 128, "some", 4),
]


def _int_draw(d, Nq, Nb, groups, seed):
    rng = np.random.default_rng(seed)
    nbase = max(1, Nb // 6)
    base = rng.integers(-1, 2, size=(nbase, d)).astype(np.float32)
    base[:, 0] = rng.integers(-8, 9, size=nbase)                  # the full range in one column
    bank = base[rng.integers(0, nbase, size=Nb)]
    Q = base[rng.integers(0, nbase, size=Nq)] + rng.integers(-1, 2, size=(Nq, d)).astype(np.float32)
    Q = np.clip(Q, -8, 8).astype(np.float32)
    qg = bg = None
    if groups != "none":
        bg = rng.integers(0, 10, size=Nb).astype(np.int32)
        qg = rng.integers(0, 10, size=Nq).astype(np.int32)
        qg[rng.random(Nq) < 0.34] = -1
        if groups == "all":
            bg[:] = 0
            qg[0] = 0
            if Nq > 2:
                qg[1], qg[2] = -1, 5
    return Q, bank.astype(np.float32), qg, bg


def int_case(d, Nq, Nb, k, groups, seed):
    """Small integers (|v| <= 8: every product and partial sum of d <= 72 terms is exact in fp32 in any order), every bank row present about
    six times (duplicated rows), the queries drawn from the bank's base rows plus noise.  groups: "none"; "some" (a third of the queries
    ungrouped (-1), the others exclude a tenth of the bank); "all" (every bank row is of group 0 and so is query 0: nothing is eligible for
    it; query 1 is ungrouped, query 2 of another group).  The draw is repeated from the next seed until at least half of the queries tie
    across the k-th place (with one or five queries a single draw can miss that), so the tie rule decides most rows that come back."""
    for s in range(seed, seed + 64):
        Q, bank, qg, bg = _int_draw(d, Nq, Nb, groups, s)
        if Nb <= k or kth_place_ties(sims_f64(Q, bank), k, qg, bg) >= 0.5:
            return Q, bank, qg, bg
    raise AssertionError("no draw with ties across the k-th place")


def unit_case(d, Nq, Nb, seed):
    """random unit-norm rows (float32), a few near-duplicates of the queries planted in the bank"""
    rng = np.random.default_rng(seed)
    bank = rng.standard_normal((Nb, d))
    Q = rng.standard_normal((Nq, d))
    for q in range(0, Nq, 3):
        bank[rng.integers(0, Nb)] = Q[q] + 1e-3 * rng.standard_normal(d)
    bank /= np.linalg.norm(bank, axis=1, keepdims=True)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return Q.astype(np.float32), bank.astype(np.float32)


def dot_bound(Q, bank, d):
    """[Nq, Nb]: d 2^-24 sum_k |a_k| |b_k| - the first-order bound of an fp32 fused multiply-add chain of d terms"""
    return d * 2.0 ** -24 * (np.abs(np.asarray(Q, np.float64)) @ np.abs(np.asarray(bank, np.float64)).T)


# ------------------------------------------------------------------ vote
def weights_ref(sim_row, k, weighting, T):
    s = np.asarray(sim_row[:k], np.float64)
    if weighting == "uniform":
        return np.ones(k, np.float64)
    with np.errstate(invalid="ignore"):
        return np.exp((s - s[0]) / np.float64(np.float32(T)))


def vote_cls_ref(idx, sim, k, weighting, T, labels, C, *, count_empty=False):
    """-> (scores float32 [Nq, C], pred int32 [Nq], scores float64).  Sums in float64 over i = 0 .. k - 1 in that order; ties to the lower class; a
    slot with idx outside [0, Nb) or a label outside [0, C) is ignored.  count_empty: the planted defect - an idx = -1 slot votes (for labels[-1])."""
    Nq, Nb = idx.shape[0], len(labels)
    sc64 = np.zeros((Nq, C), np.float64)
    pred = np.full(Nq, -1, np.int32)
    for q in range(Nq):
        w = weights_ref(sim[q], k, weighting, T)
        total, cls = 0.0, np.zeros(C, np.float64)
        for i in range(k):
            j = int(idx[q, i])
            if (j < 0 and not count_empty) or j >= Nb:
                continue
            lab = int(labels[j])
            if lab < 0 or lab >= C:
                continue
            wi = w[i] if np.isfinite(w[i]) else 1.0
            total += wi
            cls[lab] += wi
        if total > 0.0:
            sc64[q] = cls / total
            best = -1.0
            for c in range(C):
                if sc64[q, c] > best:
                    best, pred[q] = sc64[q, c], c
    return sc64.astype(np.float32), pred, sc64


def vote_reg_ref(idx, sim, k, weighting, T, targets):
    """-> (pred float32 [Nq, K], float64): the weighted mean per column over the neighbours whose target is not NaN; NaN when there is none"""
    targets = np.asarray(targets, np.float32)
    Nq, (Nb, K) = idx.shape[0], targets.shape
    out = np.full((Nq, K), np.nan, np.float64)
    for q in range(Nq):
        w = weights_ref(sim[q], k, weighting, T)
        for c in range(K):
            num = den = 0.0
            for i in range(k):
                j = int(idx[q, i])
                if j < 0 or j >= Nb or np.isnan(targets[j, c]):
                    continue
                num += w[i] * np.float64(targets[j, c])
                den += w[i]
            if den > 0.0:
                out[q, c] = num / den
    return out.astype(np.float32), out


def vote_case(Nq, Nb, kmax, C, K, seed):
    """idx / sim rows as nv_knn_topk writes them (sim descending in [-1, 1], empty slots (-1, -inf) at the end; row 1 all empty, row 2 one
    neighbour), labels with a planted two-way tie in row 0 (the lower class must win under uniform weights), targets with NaN cells and one
    neighbour (row 3's only one) whose targets are all NaN."""
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(Nb)[:kmax] for _ in range(Nq)]).astype(np.int32)
    sim = -np.sort(-rng.uniform(-1.0, 1.0, size=(Nq, kmax)), axis=1).astype(np.float32)
    fill = rng.integers(0, kmax + 1, size=Nq)
    fill[:4] = (kmax, 0, 1, 1)
    fill[4:] = np.maximum(fill[4:], 2)
    for q in range(Nq):
        idx[q, fill[q]:], sim[q, fill[q]:] = -1, -np.inf
    labels = rng.integers(0, C, size=Nb).astype(np.int32)
    assert kmax % 2 == 0 and C >= 3
    labels[idx[0, :kmax]] = np.arange(kmax) % 2 + 1      # classes 1, 2, 1, 2, ...: every even prefix is a tied vote between 1 and 2
    targets = rng.standard_normal((Nb, K)).astype(np.float32)
    targets[rng.random((Nb, K)) < 0.2] = np.nan
    targets[idx[3, 0]] = np.nan
    return idx, sim, labels, targets


# ------------------------------------------------------------------ segment mean
def segment_mean_ref(src, order, offsets):
    src = np.asarray(src, np.float32)
    G = len(offsets) - 1
    out = np.zeros((G, src.shape[1]), np.float32)
    for g in range(G):
        s = np.zeros(src.shape[1], np.float64)
        for p in range(offsets[g], offsets[g + 1]):
            s = s + src[order[p]].astype(np.float64)
        if offsets[g + 1] > offsets[g]:
            out[g] = (s / np.float64(offsets[g + 1] - offsets[g])).astype(np.float32)
    return out


def csr_of(groups, G=None):
    """host CSR of integer group ids (negative = in no segment): (order int32 [N], offsets int32 [G + 1]); rows of one segment in ascending order"""
    groups = np.asarray(groups)
    G = int(groups.max()) + 1 if G is None else G
    order, offsets = [], [0]
    for g in range(G):
        order += list(np.nonzero(groups == g)[0])
        offsets.append(len(order))
    order += [0] * (len(groups) - len(order))
    return np.asarray(order, np.int32), np.asarray(offsets, np.int32)
