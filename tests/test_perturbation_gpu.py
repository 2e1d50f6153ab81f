"""Perturbation attribution on MI355X (nv_token_ranks, nv_mask_patches, nv_class_scores, nv_curve_auc, nv_occlusion_gather; ops.token_ranks /
mask_patches / class_scores / curve_auc; NeuroEncoder.perturbation_curves / occlusion_sensitivity / attribution_volumes(method="occlusion")).

Exact gates (bit patterns through .view(torch.int32); the yardsticks are ranks_ref / mask_ref of tests/test_perturbation_cpu.py, which that file
pins to the oracle's patchify):
  token_ranks   == ranks_ref, B = 3, N in {8, 27, 125, 1000, 4096}, on ReLU / all-equal / +-0.0 / ramps / a map cut at 5 %;
  mask_patches  == mask_ref at (27, 9) with B = 3, (32, 8), (32, 2) (N = 4096) and the rectangular (8, 12, 16) / (4, 6, 8): empty, full, single-label
                and lo >= hi ranges, a source volume outside [0, B) whose sentinel-filled slot must survive, baselines 0.0 / -1.5 / per volume /
                shared, x holding NaN, +-Inf and -0.0;
  gather        ops.patch_ln_fwd of x and of x with token t masked: every row but t bit-equal, row t differs.
Gates with a tolerance:
  class_scores  "logit" bit-exact; "prob" within 2e-6 absolute of the float64 softmax (a handful of fp32 roundings on a value <= 1; the project's
                gate for values in [0, 1]); curve_auc within 1e-6 of the float64 trapezoid;
  glue          perturbation_curves / occlusion_sensitivity of the micro model against the documented job order replayed in the test
                (ops.mask_patches + model(...) chunk by chunk, scores in float64): the same gates;
  geometry      cube volumes (S = 40, cube 20, p = 8, fp32 forwards): a constant patch normalises to the patch LayerNorm's bias whatever its
                constant, so masking it with 0 changes no token - insertion reaches the unperturbed score once every non-constant patch is
                back, deletion reaches one value common to all volumes once they are gone, occlusion is zero on constant patches: 1e-4
                absolute (fp32 forwards sit at 2e-7 .. 2e-6 of the reference on logits).
Measured errors go to the parity report of test_engine_gpu.report.
"""
import pytest
import torch

import weights as W
from oracle import ref_cpu
from test_engine_gpu import report
from test_perturbation_cpu import MICRO_SIZE, mask_ref, rank_maps, ranks_ref

pytestmark = pytest.mark.gpu
PROB_TOL = 2e-6
AUC_TOL = 1e-6
GEOMETRY_TOL = 1e-4
MASK_GEOMETRIES = [(3, (27,) * 3, (9,) * 3), (2, (32,) * 3, (8,) * 3), (2, (32,) * 3, (2,) * 3), (2, (8, 12, 16), (4, 6, 8))]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    from neurovit_amd._cabi import require_gpu
    require_gpu()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def cells_of(size, patch):
    return (size[0] // patch[0]) * (size[1] // patch[1]) * (size[2] // patch[2])


# ---------------------------------------------------------------------------------------------------------------- exact comparisons

@pytest.mark.parametrize("N", [8, 27, 125, 1000, 4096])
def test_token_ranks_equal_the_stable_sort(N):
    from neurovit_amd import ops
    for name, maps in rank_maps(3, N, 3 + N).items():
        got = ops.token_ranks(maps.cuda())
        assert got.dtype == torch.int32 and got.shape == (3, N) and got.is_cuda
        assert torch.equal(got.cpu(), ranks_ref(maps)), (name, N)


def special_volume(B, size, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B,) + tuple(size), generator=g)
    flat = x.view(B, -1)
    flat[:, 0::17] = float("nan")
    flat[:, 1::19] = float("inf")
    flat[:, 2::23] = float("-inf")
    flat[:, 3::29] = -0.0
    flat[0, 5] = torch.tensor([0x7fc01234], dtype=torch.int32).view(torch.float32)[0]       # a NaN with a payload
    return x


def mask_jobs(B, N):
    rows = []
    for b in range(B):
        rows += [(b, 0, 0), (b, 0, N), (b, N // 2, N // 2 + 1), (b, 5, 3), (b, N // 3, (2 * N) // 3)]
    rows += [(B, 0, N), (0, N - 1, N), (-1, 0, N), (B - 1, 0, 1), (0, -7, 2), (B - 1, N - 2, N + 9)]
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("B,size,patch", MASK_GEOMETRIES, ids=["27p9", "32p8", "32p2", "rect"])
def test_mask_patches_equal_the_restatement(B, size, patch):
    from neurovit_amd import ops
    N = cells_of(size, patch)
    g = torch.Generator().manual_seed(N)
    x = special_volume(B, size, 71 + N)
    labels = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32)
    jobs = mask_jobs(B, N)
    J = jobs.shape[0]
    per_volume = special_volume(B, size, 72 + N).flip(1)
    shared = per_volume[-1:].clone()
    sentinel = torch.full((J,) + tuple(size), -777.25)
    for tag, baseline in (("0.0", 0.0), ("-1.5", -1.5), ("per volume", per_volume), ("shared", shared)):
        want = mask_ref(x, labels, jobs, patch, baseline, out=sentinel)
        on_device = baseline.cuda() if torch.is_tensor(baseline) else baseline
        out = sentinel.cuda()
        got = ops.mask_patches(x.cuda(), labels.cuda(), jobs.cuda(), patch if len(set(patch)) > 1 else patch[0], baseline=on_device, out=out)
        assert got.data_ptr() == out.data_ptr()
        assert torch.equal(bits(got), bits(want)), (size, patch, tag)
        for j, (b, _, _) in enumerate(jobs.tolist()):
            if not 0 <= b < B:
                assert torch.equal(bits(got[j]), bits(sentinel[j])), (tag, j)                  # nothing written
    fresh = ops.mask_patches(x.cuda(), labels.cuda(), jobs[:5].cuda(), patch)                   # `out` allocated by the call
    assert torch.equal(bits(fresh), bits(mask_ref(x, labels, jobs[:5], patch)))
    assert torch.equal(bits(fresh[0]), bits(x[0])) and torch.equal(bits(fresh[3]), bits(x[0]))    # empty range, lo >= hi: x itself


@pytest.mark.parametrize("S,p", [(27, 9), (32, 8)])
def test_masked_token_is_the_engines_token(S, p):
    from neurovit_amd import ops
    N, P = (S // p) ** 3, p ** 3
    x = W.make_volume((2, S, S, S), 73).cuda()
    gamma, beta = torch.ones(P, device="cuda"), torch.zeros(P, device="cuda")
    labels = torch.arange(N, dtype=torch.int32, device="cuda").repeat(2, 1)
    tokens = sorted({0, 1, N // 2, N - 2, N - 1})
    jobs = torch.tensor([(1, t, t + 1) for t in tokens], dtype=torch.int32, device="cuda")
    masked = ops.mask_patches(x, labels, jobs, p)

    def rows_of(vol):
        out, st = ops.patch_ln_fwd(vol.permute(0, 3, 1, 2).unsqueeze(1), p, p, p, gamma, beta)
        return out[:, :P].float().cpu().view(vol.shape[0], N, P), st.cpu().view(2, vol.shape[0], N)
    plain, plain_st = rows_of(x[1:2])
    got, got_st = rows_of(masked)
    for i, t in enumerate(tokens):
        others = [r for r in range(N) if r != t]
        assert torch.equal(bits(got[i, others]), bits(plain[0, others])), (S, t)
        assert torch.equal(bits(got_st[:, i, others]), bits(plain_st[:, 0, others])), (S, t)
        assert not torch.equal(got[i, t], plain[0, t]) and float(got[i, t].abs().max()) == 0.0      # a zero patch normalises to beta = 0


# ---------------------------------------------------------------------------------------------------------------- scores and areas

def scores_f64(logits, cls_rows, kind):
    """float64 class scores: logits [J, C] (CPU), cls_rows [J]"""
    l = logits.double()
    if kind == "logit":
        return l.gather(1, cls_rows[:, None])[:, 0]
    return torch.softmax(l, dim=1).gather(1, cls_rows[:, None])[:, 0]


def auc_f64(scores):
    s = scores.double()
    K = s.shape[1]
    return (s.sum(dim=1) - (s[:, 0] + s[:, -1]) / 2) / (K - 1)


@pytest.mark.parametrize("C", [2, 8, 125])
def test_class_scores(C):
    from neurovit_amd import ops
    g = torch.Generator().manual_seed(C)
    B, J = 5, 37
    logits = torch.randn(J, C, generator=g) * 4
    logits[3] = 80.0
    logits[3, C - 1] = -80.0
    logits[4] = -80.0
    logits[4, 0] = 80.0
    logits[5] = 0.0
    source = torch.randint(0, B, (J,), generator=g)
    jobs = torch.stack([source, torch.zeros_like(source), torch.ones_like(source)], 1).to(torch.int32)
    for cls in (torch.randint(0, C, (B,), generator=g), torch.zeros(B, dtype=torch.long), torch.full((B,), C - 1)):
        rows = cls[source]
        exact = ops.class_scores(logits.cuda(), jobs.cuda(), cls.cuda(), kind="logit")
        assert torch.equal(bits(exact), bits(logits.gather(1, rows[:, None])[:, 0]))
        prob = ops.class_scores(logits.cuda(), jobs.cuda(), cls.cuda(), kind="prob").cpu()
        err = float((prob.double() - scores_f64(logits, rows, "prob")).abs().max())
        report(f"class_scores prob C {C}: max |err| vs float64 softmax {err:.2e}")
        assert err <= PROB_TOL, (C, err)
    assert torch.equal(bits(ops.class_scores(logits.cuda(), jobs.cuda(), cls.cuda())), bits(prob))       # "prob" is the default
    with pytest.raises(ValueError, match="kind"):
        ops.class_scores(logits.cuda(), jobs.cuda(), cls.cuda(), kind="margin")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.class_scores(logits, jobs, cls)


def test_curve_auc():
    from neurovit_amd import ops
    g = torch.Generator().manual_seed(9)
    for B, K in ((1, 2), (3, 6), (4, 21), (2, 126), (70, 9)):
        scores = torch.rand(B, K, generator=g)
        got = ops.curve_auc(scores.cuda()).cpu()
        err = float((got.double() - auc_f64(scores)).abs().max())
        assert got.shape == (B,) and err <= AUC_TOL, (B, K, err)
        wide = torch.rand(B, 2 * K + 3, generator=g).cuda()                                          # strided rows: a slice of a wider table
        assert torch.equal(bits(ops.curve_auc(wide[:, K:2 * K])), bits(ops.curve_auc(wide[:, K:2 * K].contiguous())))
    assert float(ops.curve_auc(torch.ones(2, 21, device="cuda")).sub(1.0).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- module

def make_neuro(S, p, seed=81):
    from neurovit_amd.NeuroEncoder import NeuroEncoder
    torch.manual_seed(seed)
    return NeuroEncoder(W.neuro_config(S, p, DEVICE="cuda:0", **MICRO_SIZE)).eval()


def replay(model, x, labels, jobs, p, chunk, baseline=0.0):
    """the documented glue, in the test: ops.mask_patches + model(...) on consecutive slices of `chunk` jobs -> (logits [J, C], inputs [J, ...])"""
    from neurovit_amd import ops
    logits, inputs = [], []
    with torch.no_grad():
        for first in range(0, jobs.shape[0], chunk):
            masked = ops.mask_patches(x, labels, jobs[first:first + chunk].contiguous(), p, baseline=baseline)
            logits.append(model(masked).float().cpu().clone())
            inputs.append(masked.cpu())
    return torch.cat(logits), torch.cat(inputs)


@pytest.mark.parametrize("score", ["prob", "logit"])
@pytest.mark.parametrize("S,p", [(27, 9), (32, 8)])
def test_perturbation_curves_against_the_replayed_jobs(S, p, score):
    from neurovit_amd import ops
    from neurovit_amd.NeuroEncoder import perturbation_step_bounds
    model = make_neuro(S, p)
    B, N, steps, chunk = 2, (S // p) ** 3, 5, 4
    K = steps + 1
    x = W.make_volume((B, S, S, S), 82).cuda()
    _, _, maps = model.attribution_volumes(x, method="rollout", return_token_maps=True, threshold=30)
    maps = torch.where(maps >= maps.quantile(0.7, dim=1, keepdim=True), maps, torch.zeros_like(maps))     # mostly ties, as a thresholded map
    out = model.perturbation_curves(x, maps, steps=steps, chunk=chunk, score=score)
    assert sorted(out) == ["class_idx", "deletion", "deletion_auc", "fractions", "insertion", "insertion_auc", "ranks"]
    assert all(v.is_cuda for v in out.values())
    assert torch.equal(out["ranks"].cpu(), ranks_ref(maps.cpu())) and torch.equal(out["ranks"], ops.token_ranks(maps))
    assert torch.equal(out["fractions"].cpu(), (torch.arange(K).double() / steps).float())
    with torch.no_grad():
        plain = model(x).float().cpu()
    assert torch.equal(out["class_idx"].cpu(), plain.argmax(dim=1))
    m = perturbation_step_bounds(N, steps).tolist()
    rows = []
    for b in range(B):                                                            # volume-major: deletion k = 0 .. steps, then insertion
        rows += [(b, 0, m[k]) for k in range(K)] + [(b, m[k], N) for k in range(K)]
    jobs = torch.tensor(rows, dtype=torch.int32, device="cuda")
    logits, inputs = replay(model, x, out["ranks"], jobs, p, chunk)
    inputs = inputs.view(B, 2 * K, S, S, S)
    for b in range(B):
        assert torch.equal(bits(inputs[b, 0]), bits(x[b])) and torch.equal(bits(inputs[b, 2 * K - 1]), bits(x[b]))     # deletion 0, insertion `steps`
        assert float(inputs[b, K - 1].abs().max()) == 0.0 and float(inputs[b, K].abs().max()) == 0.0                   # everything removed
    cls_rows = out["class_idx"].cpu().repeat_interleave(2 * K)
    want = scores_f64(logits, cls_rows, score).view(B, 2 * K)
    tol = PROB_TOL if score == "prob" else 0.0
    for name, cols in (("deletion", slice(0, K)), ("insertion", slice(K, 2 * K))):
        err = float((out[name].cpu().double() - want[:, cols]).abs().max())
        auc_err = float((out[name + "_auc"].cpu().double() - auc_f64(out[name].cpu())).abs().max())
        report(f"perturbation_curves S{S} {score} {name}: max |err| vs replay {err:.2e}, auc {auc_err:.2e}")
        assert out[name].shape == (B, K) and out[name + "_auc"].shape == (B,)
        assert err <= tol, (name, err)
        assert auc_err <= AUC_TOL, (name, auc_err)
    for mode in ("deletion", "insertion"):
        one = model.perturbation_curves(x, maps, steps=steps, chunk=chunk, score=score, mode=mode)
        assert sorted(one) == sorted(["class_idx", "fractions", "ranks", mode, mode + "_auc"])
        err = float((one[mode].cpu().double() - want[:, slice(0, K) if mode == "deletion" else slice(K, 2 * K)]).abs().max())
        assert err <= (PROB_TOL if score == "prob" else 1e-6), (mode, err)     # (other chunk boundaries: the forward of another batch composition)


def test_perturbation_curves_targets_and_baselines():
    S, p, B = 32, 8, 2
    model = make_neuro(S, p)
    x = W.make_volume((B, S, S, S), 83).cuda()
    maps = torch.rand(B, 64, device="cuda")
    base = model.perturbation_curves(x, maps, steps=4, score="logit")
    other = 1 - base["class_idx"]
    as_tensor = model.perturbation_curves(x, maps, steps=4, score="logit", target=other)
    as_one = model.perturbation_curves(x, maps, steps=4, score="logit", target=1)
    assert torch.equal(as_tensor["class_idx"], other) and torch.equal(as_one["class_idx"], torch.ones_like(other))
    pick = (other == 1).view(B, 1)
    as_zero = model.perturbation_curves(x, maps, steps=4, score="logit", target=0)
    assert torch.equal(as_tensor["deletion"], torch.where(pick, as_one["deletion"], as_zero["deletion"]))
    # a baseline volume: inserting nothing into it, or deleting everything, leaves the baseline itself (fp32 forwards: batches of other sizes agree
    # to 2e-6 of the logits; 1e-4 as the geometry test)
    blurred = W.make_volume((1, S, S, S), 84).cuda()
    with model.precision("fp32"):
        with torch.no_grad():
            of_baseline = model(blurred).float()[0]
        exact = model.perturbation_curves(x, maps, steps=4, score="logit", baseline=blurred, chunk=3)
    for b in range(B):
        want = float(of_baseline[int(exact["class_idx"][b])])
        assert abs(float(exact["deletion"][b, -1]) - want) <= 1e-4 * max(1.0, abs(want))
        assert abs(float(exact["insertion"][b, 0]) - want) <= 1e-4 * max(1.0, abs(want))
    curves = model.perturbation_curves(x, maps, steps=4, score="logit", baseline=blurred, chunk=3)
    per_volume = model.perturbation_curves(x, maps, steps=4, score="logit", baseline=blurred.expand(B, S, S, S).contiguous(), chunk=3)
    assert torch.equal(per_volume["deletion"], curves["deletion"]) and torch.equal(per_volume["insertion"], curves["insertion"])
    assert all(q.grad is None for q in model.parameters())


@pytest.mark.parametrize("window", [1, 2])
@pytest.mark.parametrize("S,p", [(27, 9), (32, 8)])
def test_occlusion_sensitivity_against_the_replayed_jobs(S, p, window):
    from neurovit_amd import ops
    model = make_neuro(S, p)
    B, G, chunk = 2, S // p, 4
    N, Gb = G ** 3, -(-G // window)
    NB = Gb ** 3
    x = W.make_volume((B, S, S, S), 85).cuda()
    maps, cls = model.occlusion_sensitivity(x, window=window, chunk=chunk)
    assert maps.shape == (B, N) and maps.is_cuda and maps.dtype == torch.float32 and cls.shape == (B,) and cls.is_cuda
    with torch.no_grad():
        plain = model(x).float().cpu()
    assert torch.equal(cls.cpu(), plain.argmax(dim=1))
    block = torch.tensor([(c2 // window) * Gb * Gb + (c0 // window) * Gb + c1 // window for c2 in range(G) for c0 in range(G) for c1 in range(G)])
    labels = block.to(torch.int32).repeat(B, 1).cuda()
    jobs = torch.tensor([(b, j, j + 1) for b in range(B) for j in range(NB)], dtype=torch.int32, device="cuda")
    logits, inputs = replay(model, x, labels, jobs, p, chunk)
    occluded = scores_f64(logits, cls.cpu().repeat_interleave(NB), "prob").view(B, NB)
    want = scores_f64(plain, cls.cpu(), "prob")[:, None] - occluded[:, block]
    err = float((maps.cpu().double() - want).abs().max())
    report(f"occlusion_sensitivity S{S} window {window}: max |err| vs replay {err:.2e}, max |map| {float(maps.abs().max()):.2e}")
    assert err <= PROB_TOL, err
    assert float(maps.abs().max()) > 0.0                                           # a live map on random volumes
    # job j of volume b hides block j and nothing else
    zeroed = (inputs.view(B, NB, S, S, S) == 0) & (x.cpu()[:, None] != 0)
    cells = zeroed.view(B, NB, G, p, G, p, G, p).any(dim=7).any(dim=5).any(dim=3)              # [B, NB, c0, c1, c2]
    grid = block.view(G, G, G).permute(1, 2, 0)                                                # block of cell (c0, c1, c2)
    assert torch.equal(cells, (grid[None, None] == torch.arange(NB).view(1, NB, 1, 1, 1)).expand(B, NB, G, G, G))
    if window == 1:
        vols, cls_v, normalised = model.attribution_volumes(x, method="occlusion", return_token_maps=True)
        signed, _ = model.occlusion_sensitivity(x)                                  # as the method calls it: the default chunk (bf16 forwards of another batch size)
        want_vols, (want_norm, _, _) = ops.token_maps_to_volumes(torch.relu(signed), G, S, normalize=True, keep_percent=model.config["GRADCAM_THRESHOLD"],
                                                                return_maps=True)
        assert torch.equal(vols, model.token_maps_to_volumes(torch.relu(signed))) and torch.equal(vols, want_vols)
        assert torch.equal(normalised, want_norm) and torch.equal(cls_v, cls)
        assert len(model.attribution_volumes(x, method="occlusion")) == 2
        with pytest.raises(ValueError, match="method"):
            model.attribution_volumes(x, method="lime")


def test_geometry_end_to_end_on_cube_volumes():
    from neurovit_amd import synthetic
    S, cube, p = 40, 20, 8
    G = S // p
    N = G ** 3
    volumes, _, corners = synthetic.cube_volumes(16, S, cube, grid_noise=0.0, seed=5)
    distinct = []
    for i in range(volumes.shape[0]):
        if all(not torch.equal(corners[i], corners[j]) for j in distinct):
            distinct.append(i)
    assert len(distinct) >= 4
    x = volumes[distinct[:4]].contiguous()
    rows = ref_cpu.patchify(ref_cpu.fmri_to_video(x), p, p, p)                      # [4, N, p^3], token order
    live = (rows.amax(dim=2) != rows.amin(dim=2))                                  # the non-constant patches: they straddle a cube face
    count = live.sum(dim=1)
    assert bool((count > 0).all()) and bool((count < N).all())
    model = make_neuro(S, p, seed=86)
    xd = x.cuda()
    with model.precision("fp32"):
        curves = model.perturbation_curves(xd, live.float().cuda(), steps=N)        # steps = N: m_k = k
        occlusion, cls = model.occlusion_sensitivity(xd)
        with torch.no_grad():
            plain = model(xd).float().cpu()
    assert torch.equal(curves["class_idx"], cls)
    unperturbed = scores_f64(plain, cls.cpu(), "prob")
    insertion, deletion = curves["insertion"].cpu().double(), curves["deletion"].cpu().double()
    worst = dict(insertion=0.0, deletion=0.0, occlusion=0.0)
    tails = []
    for b in range(4):
        c = int(count[b])
        worst["insertion"] = max(worst["insertion"], float((insertion[b, c:] - unperturbed[b]).abs().max()))
        tails.append(deletion[b, c:])
        worst["occlusion"] = max(worst["occlusion"], float(occlusion[b].cpu()[~live[b]].abs().max()))
    # once every non-constant patch is gone the tokens of all four volumes are the same: one common score (of each volume's own class)
    same_class = [b for b in range(4) if int(cls[b]) == int(cls[0])]
    common = torch.cat([tails[b] for b in same_class])
    worst["deletion"] = float((common - common[0]).abs().max())
    with model.precision("fp32"):
        fixed = model.perturbation_curves(xd, live.float().cuda(), steps=N, target=int(cls[0]), mode="deletion")["deletion"].cpu().double()
    every = torch.cat([fixed[b, int(count[b]):] for b in range(4)])
    worst["deletion"] = max(worst["deletion"], float((every - every[0]).abs().max()))
    report(f"perturbation geometry S{S} cube {cube} p{p} fp32: insertion tail vs unperturbed {worst['insertion']:.2e}, deletion tail spread "
           f"{worst['deletion']:.2e}, occlusion on constant patches {worst['occlusion']:.2e} (live patches per volume {count.tolist()})")
    print(worst)
    assert worst["insertion"] <= GEOMETRY_TOL, worst
    assert worst["deletion"] <= GEOMETRY_TOL, worst
    assert worst["occlusion"] <= GEOMETRY_TOL, worst
    assert float(occlusion.abs().max()) > 0.0
