"""The permutation tests on the MI355X (nv_perm_design / nv_perm_stats / nv_perm_maxstat / nv_perm_finish and stats.permutation_test) held to
the numpy restatement (tests/perm_test_ref.py; what it is worth is proven in tests/test_perm_test_cpu.py).

Gates.  Integer-valued inputs make every sum exact in fp32 whatever its order, so M, a, c, max_stat, count_unc, count_fwe, max_t, critical_t and
n_invalid are BIT-equal to the restatement, p = float32(count / R), at splits 1, 3 and automatic, with NaN guard columns behind every row of
the input (ldx = V + 4) and guard cells behind every output.  The observed t lies within one fp32 ulp of float32 of scipy's double value
(double rounding can flip the last bit).  Float inputs (randn, N = 10, V = 130, R = 200): every count exact in every cell - the CPU test
asserts that no comparison of the float64 restatement lies within twice the first-order fp32 accumulation bound
(N + 2) 2^-24 sum |x_i| c(v) - and max_stat within the largest such bound of the tile's voxels (a row maximum may sit on another voxel than
the restatement's: each side's value is within its own voxel's bound).  Every figure is printed in front of its gate (run with -s).
Measured maxima on the MI355X: observed t 0 ulp from scipy in every case; float inputs max_stat 1.71e-7 from the float64 restatement under
a bound of 6.54e-7, the same at every split count; every integer quantity and every bit of the integer-valued cases exact."""
import numpy as np
import pytest
import scipy.stats
import torch

import perm_test_ref as R

pytestmark = pytest.mark.gpu

GUARD = 8
SPLITS = (1, 3, 0)
ALPHAS = (0.05, 0.01)


def note(name, value):
    print(f"measured {name}: {float(value):.3e}")


@pytest.fixture(scope="module")
def S():
    from neurovit_amd._cabi import require_gpu
    require_gpu()
    from neurovit_amd import stats
    return stats


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def guarded(n, dtype):
    """n cells in front of GUARD cells that nothing may write"""
    fill = -777 if dtype == torch.int32 else -777.0
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[:n]


def device_run(S, X, kind=R.ONE, labels=None, rows=None, tail="two", mask=None, seed=0, exact=False, splits=0):
    """the four entry points on X [N, V] stored with ldx = V + 4 (NaN in the pad columns), every output in front of guard cells"""
    N, V = X.shape
    rows = (1 << N) if exact else rows
    npad = R.npad(N)
    store = torch.full((N, V + 4), float("nan"), dtype=torch.float32, device="cuda")
    store[:, :V] = torch.from_numpy(X).cuda()
    Xd = store[:, :V]
    lab = None if labels is None else torch.from_numpy(np.asarray(labels, np.int32)).cuda()
    n_a = 0 if labels is None else int((np.asarray(labels) == 1).sum())
    md = None if mask is None else torch.from_numpy(mask).cuda()
    bufs, out = {}, {}
    for key, n, dt in (("M", rows * npad, torch.float32), ("a", V, torch.float32), ("c", V, torch.float32), ("t", V, torch.float32), ("n_invalid", 1, torch.int32),
                       ("max_stat", rows, torch.float32), ("max_t", rows, torch.float32), ("count_unc", V, torch.int32), ("count_fwe", V, torch.int32),
                       ("p_unc", V, torch.float32), ("p_fwe", V, torch.float32), ("critical_t", len(ALPHAS), torch.float32)):
        bufs[key], out[key] = guarded(n, dt)
    ws = S.perm_workspace(rows, V, splits)
    S.perm_design(kind, N, rows, labels=lab, n_a=n_a, exact=exact, seed=seed, out=out["M"])
    S.perm_stats(Xd, kind, ws, labels=lab, n_a=n_a, mask=md, out=out)
    S.perm_maxstat(Xd, out["M"].view(rows, npad), out["a"], out["c"], ws, tail=tail, splits=splits)
    S.perm_finish(kind, N, rows, V, out["c"], ws, alphas=ALPHAS, splits=splits, out=out)
    torch.cuda.synchronize()
    for key, buf in bufs.items():
        assert bool((buf[-GUARD:] == -777).all()), f"guard cells behind {key} were written"
    got = {k: host(v) for k, v in out.items()}
    got["M"] = got["M"].reshape(rows, npad)
    return got


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32))


def hold_exact(got, want, rows, what):
    """every quantity of the restatement, bit for bit (NaN payloads aside: NaN exactly where the restatement has NaN)"""
    for key in ("M", "a", "c", "max_stat", "max_t", "critical_t"):
        assert same_bits(got[key], want[key].astype(np.float32)), (what, key)
    for key in ("count_unc", "count_fwe"):
        assert np.array_equal(got[key], want[key]), (what, key, got[key], want[key])
    assert int(got["n_invalid"][0]) == want["n_invalid"], (what, got["n_invalid"], want["n_invalid"])
    valid = want["valid"]
    for key, cnt in (("p_unc", "count_unc"), ("p_fwe", "count_fwe"), ("t", None)):
        assert np.array_equal(np.isnan(got[key]), ~valid), (what, key)
        if cnt:
            assert same_bits(got[key][valid], (got[cnt][valid] / float(rows)).astype(np.float32)), (what, key)


def t_ulps(got_t, want64, valid):
    """fp32 ulps between the device's observed t and float32 of scipy's double value, over the finite entries"""
    keep = valid & np.isfinite(want64)
    if not keep.any():
        return 0.0
    want = want64[keep].astype(np.float32)
    return float((np.abs(got_t[keep].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)).max())


def scipy_t(X, kind, labels=None):
    x = X.astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == R.ONE:
            return np.asarray(scipy.stats.ttest_1samp(x, 0.0, axis=0).statistic)
        labels = np.asarray(labels)
        return np.asarray(scipy.stats.ttest_ind(x[labels == 1], x[labels == 0], axis=0, equal_var=True).statistic)


def run_all_splits(S, X, want, rows, what, **kw):
    first = None
    for splits in SPLITS:
        got = device_run(S, X, rows=rows, splits=splits, **kw)
        hold_exact(got, want, rows, f"{what} splits={splits}")
        if first is None:
            first = got
        else:      # grid independence: identical bits at every split count (t included)
            for key in got:
                assert np.array_equal(got[key].view(np.int32), first[key].view(np.int32)), (what, splits, key)
    return first


# ------------------------------------------------------------------ integer-valued inputs: bit-equal
@pytest.mark.parametrize("V", [1, 40, 65, 130])
@pytest.mark.parametrize("N", [5, 6, 9])
def test_exact_one_sample_integer_inputs_are_bit_equal(S, N, V):
    """exact enumeration (32, 64 and 512 rows); N = 5 and 9 exercise the zero pad of the K step, V the ragged and multi-tile column counts"""
    X = R.integer_case(N, V, 10 * N + V)
    want = R.run(X, exact=True, alphas=ALPHAS)
    got = run_all_splits(S, X, want, 1 << N, f"one-sample N={N} V={V}", exact=True)
    ulps = t_ulps(got["t"], scipy_t(X, R.ONE), want["valid"])
    note(f"observed t vs scipy, N={N} V={V} (fp32 ulps)", ulps)
    assert ulps <= 1.0


@pytest.mark.parametrize("V", [65, 130])
def test_random_rows_are_bit_equal(S, V):
    """N = 7, R = 100: no multiple of any row tile, and rows drawn by the hash rule"""
    X = R.integer_case(7, V, 70 + V)
    want = R.run(X, R=100, seed=5, alphas=ALPHAS)
    got = run_all_splits(S, X, want, 100, f"random rows V={V}", seed=5)
    assert t_ulps(got["t"], scipy_t(X, R.ONE), want["valid"]) <= 1.0
    other = device_run(S, X, rows=100, seed=6)
    assert np.array_equal(other["M"][0], got["M"][0]) and not np.array_equal(other["M"], got["M"])


@pytest.mark.parametrize("tail", ["two", "greater", "less"])
def test_two_samples_are_bit_equal(S, tail):
    """N = 7, n_A = 3, R = 50"""
    labels = np.array([0, 1, 0, 0, 1, 1, 0])
    X = R.integer_case(7, 130, 33)
    X[labels == 1, 0] += 3.0
    want = R.run(X, kind=R.TWO, labels=labels, R=50, seed=9, tail=tail, alphas=ALPHAS)
    got = run_all_splits(S, X, want, 50, f"two samples {tail}", kind=R.TWO, labels=labels, seed=9, tail=tail)
    assert np.all(got["M"][:, :7].sum(1) == 3) and np.array_equal(got["M"][0, :7], labels.astype(np.float32))
    ulps = t_ulps(got["t"], scipy_t(X, R.TWO, labels), want["valid"])
    note(f"two-sample observed t vs scipy, tail {tail} (fp32 ulps)", ulps)
    assert ulps <= 1.0


@pytest.mark.parametrize("N,kind", [(18, R.ONE), (40, R.TWO), (256, R.ONE)])
def test_whole_k_chunks_and_the_subject_limit_are_bit_equal(S, N, kind):
    """Npad = 20 (one 16-subject chunk of M and one quad), 40 (two chunks, two quads) and 256 (sixteen chunks, the 65 KiB slab that needs the
    raised LDS limit, four hash words per row of sign flips); R = 70 and V = 70: two row tiles and two voxel tiles, both ragged"""
    X = R.integer_case(N, 70, N)
    labels = None if kind == R.ONE else np.arange(N) % 3 == 0
    if labels is not None:
        X[labels, 0] += 2.0
        labels = labels.astype(np.int32)
    want = R.run(X, kind=kind, labels=labels, R=70, seed=N, alphas=ALPHAS)
    got = run_all_splits(S, X, want, 70, f"N={N} {kind}", kind=kind, labels=labels, seed=N)
    ulps = t_ulps(got["t"], scipy_t(X, kind, labels), want["valid"])
    note(f"observed t vs scipy, N={N} {kind} (fp32 ulps)", ulps)
    assert ulps <= 1.0


@pytest.mark.parametrize("tail", ["two", "greater", "less"])
def test_invalid_voxels_and_all_three_tails(S, tail):
    """a mask, an all-zero voxel, a constant non-zero voxel and a voxel with a NaN: NaN exactly where the restatement has it, n_invalid exact, and
    the maxima and counts of the valid voxels those of the test without the invalid ones"""
    N, V = 6, 130
    X = R.integer_case(N, V, 17)
    X[:, 3], X[:, 70], X[2, 129], X[4, 64] = 0.0, 3.0, np.nan, np.inf
    mask = np.ones(V, bool)
    mask[[7, 65, 128]] = False
    want = R.run(X, exact=True, tail=tail, mask=mask, alphas=ALPHAS)
    bad = np.zeros(V, bool)
    bad[[3, 129, 64, 7, 65, 128]] = True
    assert np.array_equal(want["valid"], ~bad) and want["n_invalid"] == 6
    got = run_all_splits(S, X, want, 1 << N, f"invalid voxels {tail}", exact=True, tail=tail, mask=mask)
    assert np.isinf(got["t"][70]) and got["t"][70] > 0 and t_ulps(got["t"], scipy_t(X, R.ONE), ~bad) <= 1.0
    alone = device_run(S, np.ascontiguousarray(X[:, ~bad]), exact=True, tail=tail)
    for key in ("max_stat", "max_t", "critical_t"):
        assert same_bits(got[key], alone[key]), key
    for key in ("count_unc", "count_fwe"):
        assert np.array_equal(got[key][~bad], alone[key]), key


# ------------------------------------------------------------------ float inputs: exact counts, bounded maxima
def test_float_inputs_counts_exact_and_maxima_within_the_bound(S):
    X = R.float_case()
    rows, seed = R.FLOAT_CASE["R"], R.FLOAT_CASE["seed"]
    want = R.run(X, R=rows, seed=seed, alphas=ALPHAS, dtype=np.float64)
    bound = float(R.accumulation_bound(X, want["c"]).max())
    first = None
    for splits in SPLITS:
        got = device_run(S, X, rows=rows, seed=seed, splits=splits)
        assert same_bits(got["M"], want["M"]) and same_bits(got["a"], want["a"]) and same_bits(got["c"], want["c"])
        assert np.array_equal(got["count_unc"], want["count_unc"]) and np.array_equal(got["count_fwe"], want["count_fwe"])      # every cell
        assert same_bits(got["p_unc"], (want["count_unc"] / float(rows)).astype(np.float32)) and same_bits(got["p_fwe"], (want["count_fwe"] / float(rows)).astype(np.float32))
        err = float(np.abs(got["max_stat"].astype(np.float64) - want["max_stat"]).max())
        note(f"float inputs, splits={splits}: max |max_stat - float64 restatement| (bound {bound:.3e})", err)
        assert err <= bound
        # the null distribution and the critical values are the transform and the order statistic of the device's own maxima
        assert same_bits(got["max_t"], R.t_of_u(got["max_stat"].astype(np.float64), R.degrees(R.ONE, 10)).astype(np.float32))
        srt = np.sort(got["max_t"])
        assert same_bits(got["critical_t"], np.array([srt[R.rank_of(al, rows) - 1] for al in ALPHAS], np.float32))
        ulps = t_ulps(got["t"], scipy_t(X, R.ONE), want["valid"])
        note("float inputs: observed t vs scipy (fp32 ulps)", ulps)
        assert ulps <= 1.0 and int(got["n_invalid"][0]) == 0
        if first is None:
            first = got
        else:
            for key in got:
                assert np.array_equal(got[key].view(np.int32), first[key].view(np.int32)), (splits, key)


# ------------------------------------------------------------------ the public call
def test_public_call_shapes_pooling_refusals_and_repeatability(S):
    from neurovit_amd import permutation_test
    N = 6
    X = R.integer_case(N, 64, 99)
    maps = torch.from_numpy(X).cuda().reshape(N, 4, 4, 4)
    want = R.run(X, exact=True, alphas=ALPHAS)
    res = permutation_test(maps)
    for key in ("t", "p_unc", "p_fwe"):
        assert tuple(res[key].shape) == (4, 4, 4) and res[key].is_cuda
    assert same_bits(host(res["p_unc"]).reshape(-1), want["p_unc"]) and same_bits(host(res["p_fwe"]).reshape(-1), want["p_fwe"])
    assert t_ulps(host(res["t"]).reshape(-1), scipy_t(X, R.ONE), want["valid"]) <= 1.0
    assert tuple(res["max_t"].shape) == (64,) and same_bits(host(res["max_t"]), want["max_t"]) and same_bits(host(res["critical_t"]), want["critical_t"])
    assert int(res["n_permutations"]) == 64 and bool(res["exact"]) and int(res["n_invalid"]) == want["n_invalid"]
    again = permutation_test(maps)
    for key in res:      # two calls: identical bits
        assert torch.equal(bits(res[key]), bits(again[key])), key
    rand = permutation_test(maps, permutations=50, exact=False, seed=3)
    assert int(rand["n_permutations"]) == 50 and not bool(rand["exact"])
    assert np.array_equal(host(rand["p_fwe"]).reshape(-1), R.run(X, R=50, seed=3)["p_fwe"], equal_nan=True)
    # subject pooling equals pooling by hand (two volumes per subject, in mixed order), with a mask and labels
    rng = np.random.default_rng(5)
    vols = torch.from_numpy(rng.integers(-4, 5, size=(12, 4, 4, 4)).astype(np.float32)).cuda()
    subjects = [0, 1, 2, 3, 4, 5, 5, 4, 3, 2, 1, 0]
    by_hand = torch.stack([((vols[i].double() + vols[11 - i].double()) / 2.0).float() for i in range(6)])
    mask = torch.ones(4, 4, 4, dtype=torch.bool, device="cuda")
    mask[0, 0, :2] = False
    labels = [0, 1, 1, 0, 1, 0]
    for kw_rows, kw_subj in ((dict(), dict()), (dict(labels=labels + labels[::-1]), dict(labels=labels))):
        pooled = permutation_test(vols, subjects=subjects, mask=mask, permutations=40, exact=False, **kw_rows)
        direct = permutation_test(by_hand, mask=mask, permutations=40, exact=False, **kw_subj)
        for key in pooled:
            assert torch.equal(bits(pooled[key]), bits(direct[key])), key
        assert int(pooled["n_invalid"]) >= 2 and bool(torch.isnan(pooled["p_fwe"][0, 0, :2]).all()) and not bool(torch.isnan(pooled["p_fwe"][1]).any())
    # refusals: mixed labels and every limit
    with pytest.raises(ValueError, match="mixed labels"):
        permutation_test(vols, subjects=subjects, labels=[0] * 11 + [1])
    for bad in (dict(maps=maps[:1]), dict(maps=torch.zeros(257, 8, device="cuda")), dict(maps=maps, permutations=(1 << 20) + 1, exact=False),
                dict(maps=torch.zeros(21, 8, device="cuda"), exact=True), dict(maps=maps, labels=[0] * 6), dict(maps=maps[:2], labels=[0, 1]),
                dict(maps=maps, labels=[0, 1, 0, 1, 0, 1], exact=True), dict(maps=maps, splits=257), dict(maps=maps, alphas=(1.5,))):
        with pytest.raises(ValueError):
            permutation_test(**bad)
    from neurovit_amd._cabi import last_error, lib
    ws = S.perm_workspace(32, 8)
    buf = torch.zeros(64, device="cuda")
    assert lib.nv_perm_stats(buf.data_ptr(), 7, 5, 8, 0, 0, None, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ws.data_ptr(), ws.numel(), None) != 0
    assert "ldx=7" in last_error()
