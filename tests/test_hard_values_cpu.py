"""tests/hard_values.py proved on the CPU: the inputs are what they claim to be, a faithful fp32 / 16-bit restatement of every kernel stays within K / 2 of float64
over all of them (each measured maximum is compared with its record in hard_values.MEASURED, from which K follows), and every planted defect lands outside K on
at least one hard input - a bound so loose that it lets one through is a failed bound.  The gates themselves run on the GPU: tests/test_hard_values_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import hard_values as hv
from conftest import rel_err, rel_l2

FMTS = ("bf16", "fp16")


def held(name, measured):
    """the restatement's maximum has not grown past its record, so it is within K / 2"""
    print(f"hard_values.MEASURED[{name!r}]: measured {measured:.4f}")
    assert measured <= hv.MEASURED[name], f"{name}: restatement at {measured:.3f} units, recorded {hv.MEASURED[name]}"
    assert measured >= 0.5 * hv.MEASURED[name], f"{name}: restatement at {measured:.3f} units, recorded {hv.MEASURED[name]}: the record is stale (K too wide)"
    assert measured <= hv.K[name] / 2


def test_every_K_is_twice_its_measured_maximum_rounded_up_to_the_next_half():
    assert hv.k_from(1.46) == 3.0 and hv.k_from(1.5) == 3.0 and hv.k_from(1.51) == 3.5 and hv.k_from(0.78) == 2.0
    for name, v in hv.MEASURED.items():
        if not name.startswith("series."):
            assert hv.K[name] == hv.k_from(v) and 2 * v <= hv.K[name] < 2 * v + 0.5
    assert hv.K["series.mean"] == hv.K["ln.mean"] and hv.K["series.rstd"] == hv.K["ln.rstd"]


# ------------------------------------------------------------------------------------------ A. GELU
def test_gelu_values_are_every_code_of_both_formats_and_the_midpoints():
    v = hv.gelu_values()
    assert v.numel() % 8 == 0
    for fmt, count in (("bf16", 65280), ("fp16", 63488)):
        c = hv.finite_codes(fmt)
        assert c.numel() == count and torch.equal(hv.to16(c, fmt), c)
        assert hv.dgelu_values(fmt).shape == (256, 256)
    fin = v[torch.isfinite(v)]
    not_bf16 = fin[hv.to16(fin, "bf16") != fin]
    mids = not_bf16[hv.to16(not_bf16, "fp16") != not_bf16]
    assert mids.numel() > 20000 and float(mids.abs().max()) < 16                    # fp32 values that are a code of neither format (most midpoints inside fp16's range are fp16 codes)
    assert int(torch.isnan(v).sum()) == 1 and int(torch.isinf(v).sum()) == 2
    # the format's spacing, subnormal floor included, against torch's own next code
    for fmt in FMTS:
        c = hv.finite_codes(fmt)
        c = torch.sort(c[c > 0]).values
        assert torch.equal(hv.ulp16(c[:-1], fmt), (c[1:].double() - c[:-1].double()))


def test_gelu_restatement_within_half_of_K_and_the_comment_in_common_h():
    v = hv.gelu_values()
    fin = v[torch.isfinite(v)]
    h = hv.gelu32(fin.numpy())
    held("gelu", float(hv.gelu_ratio(h, fin, None).max()))
    for fmt in FMTS:                                                                  # ... and no further once the 16-bit conversion and its half ulp are in
        assert float(hv.gelu_ratio(hv.to16(h, fmt), fin, fmt).max()) <= hv.K["gelu"] / 2
        c = hv.finite_codes(fmt)
        d = hv.dgelu32(c.numpy())
        held(f"dgelu.{fmt}", float(hv.gelu_ratio(d, c, None, grad=True).max()))
        assert float(hv.gelu_ratio(hv.to16(d, fmt), c, fmt, grad=True).max()) <= hv.K[f"dgelu.{fmt}"] / 2
    # what the comment above erf_parts (csrc/common.h) states: erf 5.6e-7, GELU 1.6e-7 max(1, |u|), the derivative 2.9e-7
    e, _ = hv.erf_parts32(fin.numpy())
    erf_err = float((torch.from_numpy(e).double() - torch.special.erf(fin.double() / 2 ** 0.5)).abs().max())
    assert 1.5e-7 < erf_err <= 5.6e-7
    assert float(((h.double() - hv.gelu64(fin)).abs() / fin.double().abs().clamp_min(1)).max()) <= 1.6e-7
    assert float((hv.dgelu32(fin.numpy()).double() - hv.dgelu64(fin)).abs().max()) <= 2.9e-7
    # non-finite pre-activations: NaN and +inf survive, -inf is what torch's fp32 GELU makes of it
    odd = torch.tensor([float("nan"), float("inf"), float("-inf")])
    assert hv.same_values(hv.gelu32(odd.numpy()), torch.cat([torch.nn.functional.gelu(o.reshape(1)) for o in odd]))        # (one at a time: no vector lanes)
    assert torch.isnan(hv.gelu32(odd.numpy())[0]) and hv.gelu32(odd.numpy())[1] == float("inf")


@pytest.mark.parametrize("defect", list(hv.GELU_DEFECTS))
def test_gelu_defects_land_outside_K(defect):
    kw = hv.GELU_DEFECTS[defect]
    v = hv.gelu_values()
    fin = v[torch.isfinite(v)]
    for fmt in FMTS:
        assert float(hv.gelu_ratio(hv.to16(hv.gelu32(fin.numpy(), **kw), fmt), fin, fmt).max()) > hv.K["gelu"]
        c = hv.finite_codes(fmt)
        assert float(hv.gelu_ratio(hv.to16(hv.dgelu32(c.numpy(), **kw), fmt), c, fmt, grad=True).max()) > hv.K[f"dgelu.{fmt}"]
    # ... and the gate these values used to meet (1e-3 of the largest |gelu| on randn pre-activations) lets the two coefficient defects through
    u = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 1.5
    old = float((hv.to16(hv.gelu32(u.numpy(), **kw), "bf16").double() - hv.gelu64(u)).abs().max() / hv.gelu64(u).abs().max())
    assert (old <= 1e-3 + 2.0 ** -9) == (defect != "gauss = exp(-x)")


# ------------------------------------------------------------------------------------------ B. attention
ATTN_CASES = [(n, 64) for n in hv.ATTN_SHAPES + (129,)] + [(65, 32), (130, 128)]


@functools.lru_cache(maxsize=None)
def attn_case(family, n, dh, fmt):
    qkv, do = hv.attn_qkv(family, n, fmt, dh), hv.attn_dout(n, fmt, dh)
    return qkv, do, hv.attn64(qkv, do, n, fmt, dh)


def test_attention_families_are_what_they_claim():
    for fmt in FMTS:
        for n in hv.ATTN_SHAPES:
            def probs(family):
                qkv = hv.attn_qkv(family, n, fmt)
                assert torch.equal(hv.to16(qkv, fmt), qkv)                          # 16-bit representable
                q, k, v = (hv.split_heads(t, n).double() for t in qkv.chunk(3, dim=1))
                return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1), v
            p, _ = probs("benign")
            assert 0.03 < float(p.amax(-1).mean()) < 0.15
            p, _ = probs("peaked")
            assert float(p.amax(-1).mean()) > 0.8
            p, _ = probs("late_max")
            assert bool((p.argmax(-1) == n - 1).all()) and float(p[..., -1].mean()) > 0.5         # the dominant key arrives last: a rescale in the ragged tile
            p, v = probs("sink")
            assert bool((p.argmax(-1) == 0).all()) and float(p[..., 0].mean()) > 0.5
            assert float(v[:, :, 0].abs().mean() / v[:, :, 1:].abs().mean()) > 40
            p, _ = probs("ties")
            assert float((p - 1.0 / n).abs().max()) < 1e-12
            p, v = probs("cancel")
            assert float(p.amax(-1).mean()) < 0.05 and float((p @ v).abs().max()) < 1.0 < 7.0 < float(v.abs().min())


def test_attention_restatement_within_half_of_K():
    worst = {k: 0.0 for k in ("out", "dv", "dq", "dk")}
    far = 0.0
    for fmt in FMTS:
        for family in hv.ATTN_FAMILIES:
            for n, dh in ATTN_CASES:
                qkv, do, r = attn_case(family, n, dh, fmt)
                e = hv.attn_emu(qkv, do, n, fmt, dh)
                for k in worst:
                    worst[k] = max(worst[k], float(hv.ratio(e[k], r[k], r["u_" + k]).max()))
                if family == "cancel" and fmt == "bf16":
                    far = max(far, rel_l2(e["out"], r["out"]))
    for k, v in worst.items():
        held(f"attn.{k}", v)
    assert far > 8e-3              # where the whole-tensor gates are blind: on cancelling values even the restatement is this far from float64 in rel-L2


def test_attention_defects_land_outside_K_and_what_the_old_gates_saw():
    """Each defect is outside K["attn.out"] on at least one family.  On `benign` the old gates (rel-L2 <= 1e-3 and max <= 2^-7 of the largest value, against the
    restatement) also caught all three at these n; what the per-element gate adds is the structured families, the backward, and rows a whole-tensor ratio averages away
    (on `cancel` the restatement itself is 1e-2 from float64 in rel-L2, so nothing below that was visible)."""
    caught, old_benign = {d: [] for d in hv.ATTN_DEFECTS}, {}
    for defect in hv.ATTN_DEFECTS:
        for family in hv.ATTN_FAMILIES:
            for n in hv.ATTN_SHAPES:
                qkv, do, r = attn_case(family, n, 64, "bf16")
                bad = hv.to16(hv.attn64_defect(qkv, n, defect).float(), "bf16")
                if float(hv.ratio(bad, r["out"], r["u_out"]).max()) > hv.K["attn.out"]:
                    caught[defect].append((family, n))
                if family == "benign" and n == 65:
                    emu = hv.attn_emu(qkv, do, n, "bf16")["out"]
                    old_benign[defect] = rel_l2(bad, emu) > 1e-3 or rel_err(bad, emu) > 2.0 ** -7
        assert caught[defect], defect
    fams = {d: {f for f, _ in c} for d, c in caught.items()}
    assert "ties" in fams[hv.ATTN_DEFECTS[0]] and "late_max" in fams[hv.ATTN_DEFECTS[1]] and "late_max" in fams[hv.ATTN_DEFECTS[2]]
    assert "sink" not in fams[hv.ATTN_DEFECTS[2]]          # the maximum never moves after tile 0 there: the defect is invisible on that family by construction
    assert old_benign == {d: True for d in hv.ATTN_DEFECTS}


# ------------------------------------------------------------------------------------------ C. LayerNorm
LN_KEYS = ("mean", "rstd", "dx", "dgamma", "dbeta", "colsum")


def test_row_families_are_what_they_claim():
    for d in (192, 768, 2048):
        for family in hv.ROW_FAMILIES:
            x = hv.ln_rows(family, 13, d).double()
            mean, std = x.mean(1), x.std(1, unbiased=False)
            if family == "offset":
                assert float((mean - 100).abs().max()) < 0.5 and float((std - 1).abs().max()) < 0.2
            elif family == "outlier":
                assert bool(((x == 300).sum(1) == 1).all())
            elif family == "constant":
                assert float(std.max()) == 0.0 and len(set(x[:, 0].tolist())) > 4
                r = hv.ln32(x.float(), *hv.ln_params(d))
                assert torch.equal(r["y"], hv.ln_params(d)[1].expand(13, d))       # exactly beta
            elif family == "tiny":
                assert float(std.max()) < 2e-4 and float((std ** 2).max()) < hv.LN_EPS / 100        # eps decides
            elif family == "huge":
                assert float(std.min()) > 800


def test_layernorm_restatement_within_half_of_K():
    worst = {k: 0.0 for k in LN_KEYS + ("out",)}

    def take(r32, r64, keys, fmts=()):
        for k in keys:
            worst[k] = max(worst[k], float(hv.ratio(r32[k], r64[k], r64["u_" + k]).max()))
        worst["out"] = max(worst["out"], float(hv.ratio(r32["y"], r64["y"], r64["u_y"]).max()))
        for fmt in fmts:                                                              # the 16-bit outputs, with their half ulp, add nothing
            assert float(hv.ratio(hv.to16(r32["y"], fmt), r64["y"], r64["u_y"], fmt).max()) <= hv.K["ln.out"] / 2

    for d in (192, 768, 2048):
        gamma, beta = hv.ln_params(d)
        for family in hv.ROW_FAMILIES:
            x, dy = hv.ln_rows(family, 13, d), hv.ln_rows("benign", 13, d, seed=9)
            take(hv.ln32(x, gamma, beta, dy=dy), hv.ln64(x, gamma, beta, dy=dy), LN_KEYS, FMTS)
    for p, S, vec in ((8, 16, True), (9, 18, False)):
        tok = hv.tokens_of(hv.volumes(S), p)
        gamma, beta = hv.ln_params(p ** 3)
        take(hv.ln32(tok, gamma, beta, vec=vec), hv.ln64(tok, gamma, beta), ("mean", "rstd"), FMTS)
    for S, p, T in hv.SERIES_SHAPES:
        tok = hv.series_tokens(hv.series(S, p, T), p)
        gamma, beta = hv.ln_params(p ** 3)
        take(hv.ln32(tok, gamma, beta), hv.ln64(tok, gamma, beta), ("mean", "rstd"))
    for k, v in worst.items():
        held(f"ln.{k}", v)


def test_pivot_cases_break_the_one_pass_statistics_and_not_the_centred_ones():
    """The three pivot cases: voxel 0 of every patch is the value the old kernel shifted by.  Its one-pass variance (restated in fp32) is thousands of units off on all
    three - the expected failure of the issue - and the kernel's two-round form (a first mean as the pivot, compensated final sums) sits inside the row kernels' figures."""
    worst = {"mean": 0.0, "rstd": 0.0}
    for S, p, T in hv.SERIES_SHAPES:
        x = hv.series(S, p, T)
        tok = hv.series_tokens(x, p)
        Bo, N = x.shape[0], (S // p) ** 3
        assert tok.shape == (Bo * T * N, p ** 3)
        for b, piv in enumerate((0.0, -2.5, 1000.0)):
            rows = tok.reshape(Bo, T * N, -1)[b]
            assert bool((rows[:, 0] == piv).all()) and bool((rows[:, 1:] != piv).all())
        for sigma in (None, hv.SERIES_SIGMA):
            e64, e32 = hv.series_eps(sigma, T, N)
            r64 = hv.ln64(tok, *hv.ln_params(p ** 3), eps=e64)
            mean, rstd = hv.series_stats32(tok, T, eps=e32)
            worst["mean"] = max(worst["mean"], float(hv.ratio(mean, r64["mean"], r64["u_mean"]).max()))
            worst["rstd"] = max(worst["rstd"], float(hv.ratio(rstd, r64["rstd"], r64["u_rstd"]).max()))
            _, rstd_old = hv.series_stats32(tok, T, eps=e32, old=True)
            per_case = hv.ratio(rstd_old, r64["rstd"], r64["u_rstd"]).reshape(Bo, -1).max(1).values
            assert bool((per_case > 100 * hv.K["series.rstd"]).all()), per_case              # the planted defect of this family: the kernel as it stood
            assert float(rel_err(rstd_old, r64["rstd"])) < 1e-3                               # ... which a gate at 1e-4 of the largest rstd on benign data never saw
    held("series.mean", worst["mean"])
    held("series.rstd", worst["rstd"])


# ------------------------------------------------------------------------------------------ D. AdamW
def test_adamw_inputs_and_restatement_within_half_of_K():
    worst = [0.0, 0.0, 0.0]
    for n in hv.ADAM_COUNTS:
        for start in hv.ADAM_STARTS:
            p0, grads, m0, v0 = hv.adam_inputs(n, start)
            assert 1e-4 <= float(p0.abs().min()) and float(p0.abs().max()) <= 10
            mags = torch.stack(grads).abs()
            if n >= 2044:
                for val in (0.0, 1e-12, 1e-8):
                    assert bool((mags == np.float32(val)).any(1).all())
                assert float(mags.max()) > 5 and float(mags[mags > 1e-7].min()) < 2e-4
            g3 = torch.stack(grads)
            assert not bool(((g3 > 0).any(0) & (g3 < 0).any(0)).any())                       # an element's gradient keeps its sign: m never cancels
            for wd in hv.ADAM_DECAYS:
                for gs in hv.ADAM_SCALES:
                    p, m, v = p0, m0, v0
                    for s, g in enumerate(grads):
                        ref = hv.adam64(p, g, m, v, start + s, wd, gs)
                        p, m, v = hv.adam32(p, g, m, v, start + s, wd, gs)
                        worst = [max(a, b) for a, b in zip(worst, hv.adam_ratios(p, m, v, ref))]
    for name, v in zip(("adam.p", "adam.m", "adam.v"), worst):
        held(name, v)


@pytest.mark.parametrize("defect", ["bias correction of step - 1", "eps inside the square root", "weight decay on the update instead of the parameter"])
def test_adamw_defects_land_outside_K(defect):
    """what the old gate (1e-6 of the largest |p|: 0.4 % of an update) could not see"""
    seen = 0.0
    for start in hv.ADAM_STARTS:
        p0, grads, m0, v0 = hv.adam_inputs(2052, start)
        g = grads[0]
        ref = hv.adam64(p0, g, m0, v0, start, 1e-2, 1.0)
        if defect.startswith("bias"):
            bad = hv.adam64(p0, g, m0, v0, start + 1, 1e-2, 1.0)
        elif defect.startswith("eps"):
            lr, (b1, b2), eps = hv.ADAM["lr"], hv.ADAM["betas"], hv.ADAM["eps"]
            m, v = ref[1], ref[2]
            bad = (p0.double() * (1 - lr * 1e-2) - lr / (1 - b1 ** start) * m / torch.sqrt(v / (1 - b2 ** start) + eps), m, v)
        else:
            plain = hv.adam64(p0, g, m0, v0, start, 0.0, 1.0)
            bad = (plain[0] - hv.ADAM["lr"] * 1e-2 * plain[0], plain[1], plain[2])
        seen = max(seen, hv.adam_ratios(bad[0].float(), bad[1].float(), bad[2].float(), ref)[0])
    assert seen > hv.K["adam.p"], (defect, seen)
