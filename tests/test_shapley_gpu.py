"""Shapley value sampling on MI355X (nv_shapley_ranks, nv_shapley_labels, nv_mask_patches_rows, nv_shapley_accumulate, nv_shapley_token_maps;
ops.shapley_* / mask_patches_rows; NeuroEncoder.shapley_values / attribution_volumes(method="shapley")).

Exact gates (bit patterns; the yardsticks are the restatements of tests/shapley_ref.py, which tests/test_shapley_cpu.py holds to properties of
their own):
  ranks         == draw_ref at B = 3, F in {2, 3, 8, 27, 125, 1000, 4096}, R in {1, 2}, first_unit in {0, 5};
  labels        == labels_ref with identity / block / ragged-region features, -1 cells, ids >= F, and N = 4096 with F = 7;
  masked rows   == mask_rows_ref at the geometries of the perturbation test: rows that differ from b, b or row out of range (the sentinel-filled
                slot survives), lo >= hi, float / per-volume / shared baselines, x holding NaN, +-Inf, -0.0; with row == b the bits of
                ops.mask_patches on the same jobs;
  accumulate    values, sums, delta == accumulate_ref at F in {2, 3, 125, 4096}, U in {1, 2, 7}, R in {1, 2} on scores with ties, negatives and
                a 1e4 range; stderr within 1 fp32 ulp (a double sqrt that is not correctly rounded, then one fp32 rounding, moves one ulp at most);
  token maps    == token_maps_ref; per volume they sum to the sum of the values within N 2^-24 max |value| (N fp32 divisions, each within
                2^-24 of its quotient, and the quotients of one player add up to its value).
Module:
  replay        the documented job list replayed in the test, chunk by chunk, with ops.mask_patches_rows + model(...): the returned scores equal
                the replay bit for bit (logit) or within 2e-6 (prob, the project's gate for values in [0, 1]); values / delta equal
                accumulate_ref of the returned scores bit for bit; class_idx / full_score / empty_score equal a plain forward;
  exact         F = 3 regions plus patches of no player, all 6 permutations through ranks=: the values against the exact formula over the 8
                coalition scores (each the mean of the evaluations the call returned), within 2 x (largest spread among repeated evaluations
                of one coalition, measured here) + 2^-23 max |score|: a value is an average of differences of scores and every score sits
                within the spread of its mean;
  geometry      the cube volumes of the perturbation test, fp32 forwards: constant patches are dummy players (|value| <= 1e-4), and every
                volume's values sum to full - empty within delta's bound (tests/shapley_ref.py);
  refusals, attribution_volumes(method="shapley"), token_maps into token_maps_to_volumes / perturbation_curves.
Measured errors go to the parity report of test_engine_gpu.report.
"""
import numpy as np
import pytest
import torch

import shapley_ref as SR
import weights as W
from oracle import ref_cpu
from test_engine_gpu import report
from test_perturbation_cpu import MICRO_SIZE
from test_perturbation_gpu import GEOMETRY_TOL, MASK_GEOMETRIES, PROB_TOL, bits, cells_of, make_neuro, scores_f64, special_volume

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def same_bits(got, want):
    """device tensor against a numpy array or CPU tensor of the same dtype, bit for bit (NaN payloads included)"""
    want = torch.as_tensor(want)
    got = got.detach().cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    as_int = torch.int64 if got.dtype == torch.float64 else torch.int32
    return torch.equal(got.view(as_int), want.contiguous().view(as_int))


def ulps_apart(got, want):
    """largest distance in fp32 ulps between two finite fp32 tensors of one sign"""
    a, b = got.detach().cpu().contiguous().view(torch.int32).long(), torch.as_tensor(want).contiguous().view(torch.int32).long()
    return int((a - b).abs().max())


# ---------------------------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("F", [2, 3, 8, 27, 125, 1000, 4096])
def test_shapley_ranks_equal_the_restatement(F):
    from neurovit_amd import ops
    B, U, seed = 3, 2, 77 + F
    for first_unit in (0, 5):
        for R in (1, 2):
            got = ops.shapley_ranks(U, R, B, F, seed=seed, first_unit=first_unit)
            assert got.shape == (U * R, B, F) and got.dtype == torch.int32 and got.is_cuda
            assert torch.equal(got.cpu(), SR.draw_ref(seed, first_unit, U, R, B, F)), (F, R, first_unit)
    again = ops.shapley_ranks(U, 2, B, F, seed=seed, first_unit=5)
    assert torch.equal(again, got)                                              # two runs: the same bits
    with pytest.raises(ValueError, match="shapley_ranks"):
        ops.shapley_ranks(U, 3, B, F)


def region_features(B, N, F, seed):
    """ragged regions with -1 cells and ids >= F: int32 [B, N]"""
    g = torch.Generator().manual_seed(seed)
    feats = torch.randint(0, F, (B, N), generator=g)
    feats[:, ::7] = -1
    feats[0, 1] = F
    feats[-1, 2] = F + 100
    feats[0, 3] = -5
    return feats.to(torch.int32)


def test_shapley_labels_equal_the_restatement():
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import window_block_labels
    g = torch.Generator().manual_seed(5)
    cases = []
    for B, N, F, features in ((2, 27, 27, torch.arange(27, dtype=torch.int32).repeat(2, 1)),                     # identity: one player per patch
                              (3, 64, 8, window_block_labels(4, 2).to(torch.int32).repeat(3, 1)),               # blocks
                              (2, 125, 27, window_block_labels(5, 2).to(torch.int32).repeat(2, 1)),             # ragged last blocks
                              (3, 125, 11, region_features(3, 125, 11, 6)),
                              (2, 4096, 7, region_features(2, 4096, 7, 7))):
        for Q in (1, 3):
            ranks = torch.stack([torch.stack([torch.randperm(F, generator=g) for _ in range(B)]) for _ in range(Q)]).to(torch.int32)
            cases.append((ranks, features.contiguous()))
    for ranks, features in cases:
        got = ops.shapley_labels(ranks.cuda(), features.cuda())
        want = SR.labels_ref(ranks, features)
        assert got.dtype == torch.int32 and torch.equal(got.cpu(), want), (ranks.shape, features.shape)
        flat = ops.shapley_labels(ranks.view(-1, ranks.shape[-1]).cuda(), features.cuda())                       # [Q B, F] is the same table
        assert torch.equal(flat, got)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shapley_labels(ranks, features)


def row_jobs(B, Rows, N):
    rows = []
    for b in range(B):
        other = (b + 1) % Rows
        rows += [(b, b, 0, 0), (b, other, 0, N), (b, other, N // 2, N // 2 + 1), (b, other, 1, N), (b, other, 2, N), (b, Rows - 1, 5, 3),
                 (b, b, N // 3, (2 * N) // 3)]
    rows += [(B, 0, 0, N), (0, Rows, 0, N), (0, -1, 0, N), (-1, 0, 0, N), (0, Rows - 1, N - 1, N), (B - 1, 0, -7, 2), (B - 1, 1, N - 2, N + 9)]
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("B,size,patch", MASK_GEOMETRIES, ids=["27p9", "32p8", "32p2", "rect"])
def test_mask_patches_rows_equal_the_restatement(B, size, patch):
    from neurovit_amd import ops
    N = cells_of(size, patch)
    Rows = 2 * B + 1
    g = torch.Generator().manual_seed(N)
    x = special_volume(B, size, 91 + N)
    labels = torch.stack([torch.randperm(N, generator=g) for _ in range(Rows)]).to(torch.int32)
    labels[Rows - 1, ::5] = N                                                  # patches of no player
    jobs = row_jobs(B, Rows, N)
    J = jobs.shape[0]
    per_volume = special_volume(B, size, 92 + N).flip(1)
    shared = per_volume[-1:].clone()
    sentinel = torch.full((J,) + tuple(size), -777.25)
    small = patch if len(set(patch)) > 1 else patch[0]
    for tag, baseline in (("0.0", 0.0), ("-1.5", -1.5), ("per volume", per_volume), ("shared", shared)):
        want = SR.mask_rows_ref(x, labels, jobs, patch, baseline, out=sentinel)
        on_device = baseline.cuda() if torch.is_tensor(baseline) else baseline
        out = sentinel.cuda()
        got = ops.mask_patches_rows(x.cuda(), labels.cuda(), jobs.cuda(), small, baseline=on_device, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(bits(got), bits(want)), (size, patch, tag)
        for j, (b, row, _, _) in enumerate(jobs.tolist()):
            if not (0 <= b < B and 0 <= row < Rows):
                assert torch.equal(bits(got[j]), bits(sentinel[j])), (tag, j)                  # nothing written
    assert torch.equal(bits(got[0]), bits(x[0])) and torch.equal(bits(got[5]), bits(x[0]))     # empty range, lo >= hi: x itself
    # with row == b: the bits of nv_mask_patches on the same jobs
    same = torch.tensor([(b, lo, hi) for b in range(B) for lo, hi in ((0, N), (3, 3), (N // 4, N // 2), (0, 1))] + [(B, 0, N)], dtype=torch.int32)
    rows4 = torch.stack([same[:, 0], same[:, 0], same[:, 1], same[:, 2]], 1).contiguous()
    fill = torch.full((same.shape[0],) + tuple(size), 3.5)
    for baseline in (0.0, per_volume.cuda(), shared.cuda()):
        a = ops.mask_patches(x.cuda(), labels[:B].contiguous().cuda(), same.cuda(), small, baseline=baseline, out=fill.cuda())
        b4 = ops.mask_patches_rows(x.cuda(), labels[:B].contiguous().cuda(), rows4.cuda(), small, baseline=baseline, out=fill.cuda())
        assert torch.equal(bits(a), bits(b4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_patches_rows(x, labels, jobs, small)


def accumulate_case(F, U, R, B, seed):
    """scores with ties, negatives and a 1e4 range: (interior [U R, B, F - 1], ends [B, 2], ranks [U R, B, F])"""
    g = torch.Generator().manual_seed(seed)
    Q = U * R
    interior = torch.randn(Q, B, F - 1, generator=g) * torch.tensor([1.0, 1e2, 1e4][:B]).view(1, B, 1)
    interior[:, :, ::3] = interior[:, :, :1].clone()                            # ties: zero marginals
    interior[:, 0, ::4] = 0.25
    ends = torch.randn(B, 2, generator=g) * torch.tensor([1.0, 1e2, 1e4][:B]).view(B, 1)
    ranks = torch.stack([torch.stack([torch.randperm(F, generator=g) for _ in range(B)]) for _ in range(Q)]).to(torch.int32)
    if R == 2:
        ranks[1::2] = F - 1 - ranks[0::2]
    return interior.contiguous(), ends.contiguous(), ranks.contiguous()


@pytest.mark.parametrize("F", [2, 3, 125, 4096])
def test_shapley_accumulate_equals_the_restatement(F):
    from neurovit_amd import ops
    B = 3
    worst = 0
    for U in (1, 2, 7):
        for R in (1, 2):
            interior, ends, ranks = accumulate_case(F, U, R, B, 1000 * F + 10 * U + R)
            values, stderr, delta, sums = ops.shapley_accumulate(interior.cuda(), ends.cuda(), ranks.cuda(), R=R)
            w_values, w_stderr, w_delta, w_sums = SR.accumulate_ref(interior, ends, ranks, R)
            assert same_bits(sums, w_sums), (F, U, R)
            assert same_bits(values, w_values), (F, U, R)
            assert same_bits(delta, w_delta), (F, U, R)
            M = [float(max(interior[:, b].abs().max(), ends[b].abs().max())) for b in range(B)]
            assert all(abs(float(w_delta[b])) <= SR.delta_bound(M[b], F, U) for b in range(B)), (F, U, R, w_delta, M)
            if U == 1:
                assert bool(torch.isnan(stderr).all()) and np.isnan(w_stderr).all()
            else:
                assert bool((stderr >= 0).all()) and (w_stderr >= 0).all()
                worst = max(worst, ulps_apart(stderr, w_stderr))
            again = ops.shapley_accumulate(interior.cuda(), ends.cuda(), ranks.cuda(), R=R)
            assert all(same_bits(a, b.cpu()) for a, b in zip(again[:1] + again[2:], (values, delta, sums)))    # two runs: the same bits
    report(f"shapley_accumulate F {F}: stderr within {worst} fp32 ulp of the float64 restatement")
    assert worst <= 1, worst


def test_shapley_token_maps_equal_the_restatement():
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import window_block_labels
    g = torch.Generator().manual_seed(8)
    for B, N, F, features in ((2, 27, 27, torch.arange(27, dtype=torch.int32).repeat(2, 1)),
                              (3, 125, 27, window_block_labels(5, 2).to(torch.int32).repeat(3, 1)),
                              (3, 125, 11, region_features(3, 125, 11, 9)),
                              (2, 4096, 7, region_features(2, 4096, 7, 10)),
                              (2, 4096, 4096, torch.stack([torch.randperm(4096, generator=g) for _ in range(2)]).to(torch.int32))):
        values = (torch.randn(B, F, generator=g) * 3).contiguous()
        features = features.contiguous()
        got = ops.shapley_token_maps(values.cuda(), features.cuda())
        want = SR.token_maps_ref(values, features)
        assert same_bits(got, want), (B, N, F)
        for b in range(B):
            present = torch.unique(features[b][(features[b] >= 0) & (features[b] < F)]).long()
            err = abs(float(got[b].cpu().double().sum() - values[b][present].double().sum()))
            assert err <= N * 2.0 ** -24 * float(values[b].abs().max()), (B, N, F, err)


# ---------------------------------------------------------------------------------------------------------------- module

def job_list(B, F, P):
    """the documented global order: the ends volume-major, then permutation q, volume b, k = 1 .. F - 1"""
    rows = []
    for b in range(B):
        rows += [(b, b, 0, F), (b, b, F, F)]
    for q in range(P):
        for b in range(B):
            rows += [(b, q * B + b, k, F) for k in range(1, F)]
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("score", ["prob", "logit"])
@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("S,p", [(27, 9), (32, 8)])
def test_shapley_values_against_the_replayed_jobs(S, p, window, score):
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import window_block_labels
    model = make_neuro(S, p)
    B, G, P, chunk, seed, offset = 2, S // p, 4, 4, 3, 5
    N, F = G ** 3, (-(-G // window)) ** 3
    x = W.make_volume((B, S, S, S), 87).cuda()
    out = model.shapley_values(x, permutations=P, window=window, chunk=chunk, score=score, seed=seed, permutation_offset=offset, return_scores=True)
    assert sorted(out) == ["class_idx", "delta", "empty_score", "ends", "feature_labels", "full_score", "interior", "ranks", "stderr", "token_maps", "values"]
    assert all(v.is_cuda for v in out.values())
    assert out["values"].shape == (B, F) and out["stderr"].shape == (B, F) and out["token_maps"].shape == (B, N) and out["delta"].shape == (B,)
    assert out["interior"].shape == (P, B, F - 1) and out["ends"].shape == (B, 2)
    features = window_block_labels(G, window).to(torch.int32).repeat(B, 1)
    assert torch.equal(out["feature_labels"].cpu(), features)
    ranks = SR.draw_ref(seed, offset, P // 2, 2, B, F)                          # antithetic: P / 2 units of two rows
    assert torch.equal(out["ranks"].cpu(), ranks)
    labels = SR.labels_ref(ranks, features)
    assert torch.equal(ops.shapley_labels(out["ranks"], out["feature_labels"]).cpu(), labels)
    with torch.no_grad():
        plain = model(x).float().cpu()
    assert torch.equal(out["class_idx"].cpu(), plain.argmax(dim=1))
    # the replay
    jobs = job_list(B, F, P).cuda()
    logits = []
    with torch.no_grad():
        for first in range(0, jobs.shape[0], chunk):
            masked = ops.mask_patches_rows(x, labels.cuda(), jobs[first:first + chunk].contiguous(), p)
            logits.append(model(masked).float().cpu().clone())
    logits = torch.cat(logits)
    cls_rows = out["class_idx"].cpu()[jobs[:, 0].cpu().long()]
    want = scores_f64(logits, cls_rows, score)
    got = torch.cat([out["ends"].reshape(-1), out["interior"].reshape(-1)]).cpu()
    err = float((got.double() - want).abs().max())
    report(f"shapley_values S{S} window {window} {score}: max |err| vs replay {err:.2e} over {jobs.shape[0]} jobs")
    assert err <= (PROB_TOL if score == "prob" else 0.0), err
    # the ends against a plain forward of the same four volumes in the batch of the first chunk: everything at the baseline, x itself
    with torch.no_grad():
        four = torch.stack([torch.zeros_like(x[0]), x[0], torch.zeros_like(x[1]), x[1]])
        ends_plain = scores_f64(model(four).float().cpu(), out["class_idx"].cpu().repeat_interleave(2), score).view(B, 2)
    ends_err = float((out["ends"].cpu().double() - ends_plain).abs().max())
    assert ends_err <= (PROB_TOL if score == "prob" else 0.0), ends_err
    assert torch.equal(out["empty_score"], out["ends"][:, 0]) and torch.equal(out["full_score"], out["ends"][:, 1])
    # values, delta: the restatement applied to the returned scores, bit for bit
    w_values, w_stderr, w_delta, _ = SR.accumulate_ref(out["interior"].cpu(), out["ends"].cpu(), ranks, 2)
    assert same_bits(out["values"], w_values) and same_bits(out["delta"], w_delta)
    assert ulps_apart(out["stderr"], w_stderr) <= 1
    assert same_bits(out["token_maps"], SR.token_maps_ref(torch.from_numpy(w_values), features))
    M = float(got.abs().max())
    assert float(out["delta"].abs().max()) <= SR.delta_bound(M, F, P // 2)
    assert float(out["values"].abs().max()) > 0.0                               # live values on random volumes
    assert all(q.grad is None for q in model.parameters())


def test_exact_shapley_values_of_three_regions():
    S, p, B, F = 32, 8, 2, 3
    N = (S // p) ** 3
    model = make_neuro(S, p)
    x = W.make_volume((B, S, S, S), 88).cuda()
    g = torch.Generator().manual_seed(12)
    features = torch.randint(0, F, (N,), generator=g)
    features[::9] = -1                                                         # patches of no player
    rows = SR.all_rank_rows(F)
    for score in ("prob", "logit"):
        out = model.shapley_values(x, features=features, ranks=rows, score=score, return_scores=True)
        assert torch.equal(out["ranks"].cpu(), rows[:, None, :].expand(6, B, F)) and out["values"].shape == (B, F)
        assert torch.equal(out["feature_labels"].cpu(), features.to(torch.int32).expand(B, N))
        interior, ends, values = out["interior"].cpu().double(), out["ends"].cpu().double(), out["values"].cpu().double()
        worst, spread, top = 0.0, 0.0, 0.0
        for b in range(B):
            seen = {0: [float(ends[b, 0])], (1 << F) - 1: [float(ends[b, 1])]}
            for q, r in enumerate(rows.tolist()):
                for k in range(1, F):
                    seen.setdefault(sum(1 << f for f in range(F) if r[f] < k), []).append(float(interior[q, b, k - 1]))
            assert len(seen) == 1 << F
            spread = max(spread, max(max(v) - min(v) for v in seen.values()))
            top = max(top, max(abs(s) for v in seen.values() for s in v))
            exact = SR.exact_shapley([float(np.mean(seen[m])) for m in range(1 << F)])
            worst = max(worst, float(np.abs(values[b].numpy() - exact).max()))
        tol = 2 * spread + 2.0 ** -23 * top
        report(f"shapley_values exact F 3 {score}: max |value - exact| {worst:.2e}, spread among repeated evaluations {spread:.2e}, tolerance {tol:.2e}")
        assert worst <= tol, (score, worst, spread, tol)
        assert float(values.abs().max()) > 10 * tol                            # the check bites: the values are well above it
        # a patch of no player is never masked: the everything-at-baseline copy keeps them
        assert float(out["token_maps"].cpu()[:, features < 0].abs().max()) == 0.0


def test_geometry_on_cube_volumes():
    from neurovit_amd import synthetic
    S, cube, p = 40, 20, 8
    G = S // p
    N = G ** 3
    volumes, _, corners = synthetic.cube_volumes(16, S, cube, grid_noise=0.0, seed=5)
    distinct = []
    for i in range(volumes.shape[0]):
        if all(not torch.equal(corners[i], corners[j]) for j in distinct):
            distinct.append(i)
    x = volumes[distinct[:4]].contiguous()
    rows = ref_cpu.patchify(ref_cpu.fmri_to_video(x), p, p, p)
    live = (rows.amax(dim=2) != rows.amin(dim=2))                              # the non-constant patches
    assert bool((live.sum(dim=1) > 0).all()) and bool((live.sum(dim=1) < N).all())
    model = make_neuro(S, p, seed=86)
    P = 2
    with model.precision("fp32"):
        out = model.shapley_values(x.cuda(), window=1, permutations=P, seed=1, return_scores=True)
    values = out["values"].cpu()
    assert values.shape == (4, N)
    dummy = float(values[~live].abs().max())
    M = float(max(out["interior"].abs().max(), out["ends"].abs().max()))
    bound = SR.delta_bound(M, N, P // 2)
    delta = float(out["delta"].abs().max())
    total = float((values.double().sum(dim=1) - (out["full_score"].cpu().double() - out["empty_score"].cpu().double())).abs().max())
    report(f"shapley geometry S{S} cube {cube} p{p} fp32: |value| on constant patches {dummy:.2e}, |delta| {delta:.2e} (bound {bound:.2e}), "
           f"|sum of the fp32 values - (full - empty)| {total:.2e}, max |value| {float(values.abs().max()):.2e}")
    assert dummy <= GEOMETRY_TOL, dummy
    assert delta <= bound, (delta, bound)
    assert total <= bound + N * 2.0 ** -24 * M, (total, bound)                # every fp32 value within 2^-25 |value| <= 2^-24 M of its double
    assert float(values[live].abs().max()) > 0.0


def test_refusals(tmp_path):
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    S, p, B = 32, 8, 2
    model = make_neuro(S, p)
    x = W.make_volume((B, S, S, S), 89).cuda()
    N = 64
    three = torch.arange(N) % 3
    rows = SR.all_rank_rows(3)
    with pytest.raises(ValueError, match="even"):
        model.shapley_values(x, permutations=3)
    with pytest.raises(ValueError, match="players"):
        model.shapley_values(x, window=4)                                      # one block
    with pytest.raises(ValueError, match="players"):
        model.shapley_values(x, features=torch.zeros(N, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="features name player 2"):
        model.shapley_values(x, features=three.cuda(), ranks=rows[:, :2] % 2)
    for wrong in (rows[0], rows[:, None, :].expand(6, 3, 3), rows.float()):
        with pytest.raises(ValueError, match="ranks must be"):
            model.shapley_values(x, features=three, ranks=wrong)
    broken = rows.clone()
    broken[4, 1] = broken[4, 0]
    for wrong in (broken, rows + 1, broken[:, None, :].expand(6, B, 3)):
        with pytest.raises(ValueError, match="permutation of 0 .. 2"):
            model.shapley_values(x, features=three, ranks=wrong)
    with pytest.raises(ValueError, match="label cells"):
        model.shapley_values(x, window=1, permutations=2 ** 20)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shapley_accumulate(torch.zeros(2, 1, 2), torch.zeros(1, 2), torch.zeros(2, 1, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shapley_token_maps(torch.zeros(1, 3), torch.zeros(1, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.shapley_ranks(1, 1, 1, 3, device="cpu")
    torch.save(model.state_dict(), tmp_path / "c.pth")
    four_d = NeuroEncoder(W.neuro_config(S, p, dim=4, DEVICE="cuda:0", GLOBAL_BASE_PATH=str(tmp_path), BEST_MODEL_PATH="c.pth", **MICRO_SIZE))
    with pytest.raises(NotImplementedError, match="3D model only"):
        four_d.shapley_values(x)


def test_downstream_volumes_and_curves():
    S, p, B = 32, 8, 2
    model = make_neuro(S, p)
    x = W.make_volume((B, S, S, S), 90).cuda()
    result = model.shapley_values(x)
    again = model.shapley_values(x)
    assert all(torch.equal(bits(result[k]), bits(again[k])) for k in ("values", "stderr", "delta", "token_maps", "ranks"))      # two runs: the same bits
    assert result["values"].shape == (B, 8) and result["ranks"].shape == (16, B, 8)
    other = model.shapley_values(x, permutation_offset=8)                      # disjoint units: other permutations
    assert not torch.equal(other["ranks"], result["ranks"])
    volumes, class_idx, normalised = model.attribution_volumes(x, method="shapley", return_token_maps=True)
    assert volumes.shape == (B, S, S, S) and volumes.is_cuda and volumes.dtype == torch.float32
    assert torch.equal(class_idx, result["class_idx"])
    assert torch.equal(volumes, model.token_maps_to_volumes(torch.relu(result["token_maps"])))
    target = 1 - result["class_idx"]
    assert torch.equal(model.attribution_volumes(x, method="shapley", target=target)[1], target)
    curves = model.perturbation_curves(x, result["token_maps"], steps=4)
    assert curves["deletion"].shape == (B, 5) and bool(torch.isfinite(curves["deletion_auc"]).all())
