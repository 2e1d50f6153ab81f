"""What tests/perm_test_ref.py (the numpy restatement of csrc/perm_test.hip) is worth: its u form against scipy's t tests row by row, its exact
p-values against a plain loop over all sign flips, its row rules, a planted signal, and the premise of the float-input GPU case (no comparison
within twice the fp32 accumulation bound).  Plus what needs no GPU of the feature itself: the binding, the host-side refusals, the host-check
program under the host sanitizers and the refusals of stats.permutation_test."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.stats
import torch

import perm_test_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


def u_double(X, M, kind, labels=None):
    """u of every row and voxel in double throughout (no fp32 constant), and the amplification of its rounding errors (below)"""
    X = X.astype(np.float64)
    N = X.shape[0]
    S = M[:, :N].astype(np.float64) @ X
    T, Q, A = X.sum(0), (X * X).sum(0), np.abs(X).sum(0)
    if kind == R.ONE:
        a, c = np.zeros_like(T), 1.0 / np.sqrt(N * Q)
    else:
        n_a = int((np.asarray(labels) == 1).sum())
        a, c = n_a * T / N, 1.0 / np.sqrt(n_a * (N - n_a) * (Q - T * T / N) / N)
        A = A + np.abs(a) + np.sqrt(N * Q)      # SS = Q - T^2 / N is itself a difference: its error enters c
    u = (S - a[None, :]) * c[None, :]
    return u, (A * c)[None, :] / np.maximum(np.abs(u), 1e-300)


def t_gate(u, amp, N):
    """The gate of |t_ref - t_scipy| / |t|, derived: u = (S - a) c carries at most (N + 2) roundings of relative size 2^-53 on magnitudes below
    A = sum |x_i| (+ |a|), so |du| / |u| <= (N + 2) eps A c / |u| = (N + 2) eps amp; d ln t / d ln u = 1 / (1 - u^2) (t = u sqrt(df / (1 - u^2)));
    the transform adds 4 roundings.  scipy's mean / variance route has errors of the same kind and size, so the gate is twice that of one side."""
    return 2.0 * ((N + 2) * amp / (1.0 - u * u) + 4.0) * EPS


# ------------------------------------------------------------------ the u form against scipy
@pytest.mark.parametrize("N", [4, 5, 6])
def test_exact_one_sample_rows_equal_scipy_ttest_1samp(N):
    rng = np.random.default_rng(40 + N)
    X = (rng.standard_normal((N, 7)) + 0.4).astype(np.float32)
    M = R.design(R.ONE, N, 1 << N, exact=True)
    u, amp = u_double(X, M, R.ONE)
    t = R.t_of_u(u, R.degrees(R.ONE, N))
    worst = 0.0
    for r in range(1 << N):
        want = scipy.stats.ttest_1samp(M[r, :N, None].astype(np.float64) * X.astype(np.float64), 0.0, axis=0).statistic
        err = np.abs(t[r] - want) / np.abs(want) / t_gate(u[r], amp[r], N)
        worst = max(worst, float(err.max()))
    print(f"measured one-sample |t - scipy| over its gate, N = {N}: {worst:.3f}")
    assert worst <= 1.0
    for v in range(X.shape[1]):      # the ordering by u is the ordering by t
        order = np.argsort(u[:, v], kind="stable")
        assert np.all(np.diff(t[order, v]) >= 0.0)
        assert np.array_equal(np.diff(u[order, v]) > 0.0, np.diff(t[order, v]) > 0.0)


def test_two_sample_rows_equal_scipy_ttest_ind():
    N, n_a, rows = 7, 3, 50
    rng = np.random.default_rng(7)
    X = (rng.standard_normal((N, 6)) + 1.0).astype(np.float32)
    labels = np.array([1, 0, 0, 1, 0, 1, 0])
    M = R.design(R.TWO, N, rows, seed=5, labels=labels)
    u, amp = u_double(X, M, R.TWO, labels)
    t = R.t_of_u(u, R.degrees(R.TWO, N))
    worst = 0.0
    for r in range(rows):
        m = M[r, :N] == 1
        want = scipy.stats.ttest_ind(X[m].astype(np.float64), X[~m].astype(np.float64), axis=0, equal_var=True).statistic
        worst = max(worst, float((np.abs(t[r] - want) / np.abs(want) / t_gate(u[r], amp[r], N)).max()))
    print(f"measured two-sample |t - scipy| over its gate: {worst:.3f}")
    assert worst <= 1.0
    for v in range(X.shape[1]):
        order = np.argsort(u[:, v], kind="stable")
        assert np.all(np.diff(t[order, v]) >= 0.0)


def test_observed_t_of_the_restatement_is_scipys():
    rng = np.random.default_rng(1)
    X = (rng.standard_normal((9, 33)) + 0.3).astype(np.float32)
    one = R.stats(X, R.ONE)
    want = scipy.stats.ttest_1samp(X.astype(np.float64), 0.0, axis=0).statistic
    assert np.all(np.abs(one["t"].astype(np.float64) - want.astype(np.float32)) <= np.spacing(np.abs(want.astype(np.float32))))
    labels = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0])
    two = R.stats(X, R.TWO, labels)
    want = scipy.stats.ttest_ind(X[labels == 1].astype(np.float64), X[labels == 0].astype(np.float64), axis=0, equal_var=True).statistic
    assert np.all(np.abs(two["t"].astype(np.float64) - want.astype(np.float32)) <= np.spacing(np.abs(want.astype(np.float32))))


# ------------------------------------------------------------------ exact p-values
@pytest.mark.parametrize("tail", ["two", "greater", "less"])
def test_exact_p_values_equal_a_plain_loop_over_all_sign_flips(tail):
    N, V = 6, 9
    rng = np.random.default_rng(60)
    X = (rng.standard_normal((N, V)) + 0.5).astype(np.float32)
    X[:, 0] = np.abs(X[:, 0]) + 1.0      # every subject positive: the observed labelling is the single most extreme one
    res = R.run(X, exact=True, tail=tail)
    x = X.astype(np.float64)

    def t_plain(sample):
        return sample.mean(0) / np.sqrt(sample.var(0, ddof=1) / N)

    def stat(t):
        return np.abs(t) if tail == "two" else (t if tail == "greater" else -t)

    flips = [np.array(s)[:, None] for s in itertools.product((1.0, -1.0), repeat=N)]
    t_all = np.stack([stat(t_plain(s * x)) for s in flips])
    t_obs = stat(t_plain(x))
    close = np.abs(t_all - t_obs[None, :]) <= 1e-9 * np.abs(t_obs)[None, :]      # the mirrored flip: equal |t| up to the rounding of this loop
    count_unc = ((t_all >= t_obs[None, :]) | close).sum(0)
    top = t_all.max(1)
    count_fwe = ((top[:, None] >= t_obs[None, :]) | (np.abs(top[:, None] - t_obs[None, :]) <= 1e-9 * np.abs(t_obs)[None, :])).sum(0)
    assert np.array_equal(res["count_unc"], count_unc) and np.array_equal(res["count_fwe"], count_fwe)
    rows = 1 << N
    assert np.array_equal(res["p_unc"], (count_unc / rows).astype(np.float32)) and np.array_equal(res["p_fwe"], (count_fwe / rows).astype(np.float32))
    assert np.all(res["p_fwe"] >= res["p_unc"]) and res["p_unc"].min() >= 1.0 / rows
    if tail == "greater":
        assert res["p_unc"][0] == np.float32(1.0 / rows) and res["p_unc"].min() == np.float32(1.0 / rows)      # min p = 1 / R: row 0 alone
    if tail == "two":
        assert res["count_unc"][0] == 2      # ... and its mirror image under two tails


def test_critical_value_is_the_order_statistic_found_by_counting():
    rng = np.random.default_rng(2)
    res = R.run(rng.standard_normal((8, 20)).astype(np.float32), exact=True, alphas=(0.05, 0.01, 0.5))
    for al, crit in zip((0.05, 0.01, 0.5), res["critical_t"]):
        k = int(np.ceil(round((1.0 - al) * 256, 9)))
        at_most = res["max_t"][res["max_t"] <= crit]
        assert R.rank_of(al, 256) == k and len(at_most) >= k and (res["max_t"] < crit).sum() < k and crit in res["max_t"]
    assert [R.rank_of(0.05, n) for n in (100, 32, 10000)] == [95, 31, 9500] and R.rank_of(0.29, 100) == 71


# ------------------------------------------------------------------ row rules
def test_row_rules():
    for N in (5, 8):
        M = R.design(R.ONE, N, 1 << N, exact=True)
        assert M.shape == (1 << N, R.npad(N)) and np.all(M[0, :N] == 1.0) and np.all(M[:, N:] == 0.0) and np.all(np.abs(M[:, :N]) == 1.0)
        assert len({tuple(row) for row in M}) == 1 << N      # every sign pattern once
        assert np.array_equal(M[5, :N] < 0, [(5 >> i) & 1 == 1 for i in range(N)])
    M1, M2 = R.design(R.ONE, 70, 40, seed=1), R.design(R.ONE, 70, 40, seed=2)      # two hash words per row
    assert M1.shape == (40, 72) and np.all(M1[0, :70] == 1.0) and np.all(M1[:, 70:] == 0.0) and np.all(np.abs(M1[:, :70]) == 1.0)
    assert not np.array_equal(M1, M2) and np.array_equal(M1, R.design(R.ONE, 70, 40, seed=1))
    assert abs(float(M1[1:, :70].mean())) < 0.1      # fair signs
    assert M1[3, 65] == (-1.0 if (R.hash64(1 ^ R.D1, 3 * 2 + 1) >> 1) & 1 else 1.0)
    labels = np.array([0, 1, 1, 0, 0, 1, 0])
    T1, T2 = R.design(R.TWO, 7, 50, seed=1, labels=labels), R.design(R.TWO, 7, 50, seed=2, labels=labels)
    assert np.array_equal(T1[0, :7], labels.astype(np.float32)) and np.all(T1[:, 7:] == 0.0)
    assert np.all(T1[:, :7].sum(1) == 3) and np.all((T1 == 0) | (T1 == 1)) and not np.array_equal(T1, T2)
    assert len({tuple(row) for row in T1}) > 20      # of the 35 labellings


# ------------------------------------------------------------------ a planted signal
PLANTED_NULL_UNDER_005 = 0      # recorded for the seed below: null voxels with p_fwe < 0.05 (the FWE level promises at most one such map in twenty)


def test_planted_signal_is_found_with_the_error_controlled():
    N, V = 12, 200
    rng = np.random.default_rng(12)
    X = rng.standard_normal((N, V)).astype(np.float32)
    X[:, :10] += 3.0
    res = R.run(X, exact=True)      # 4096 rows
    assert np.all(res["p_fwe"][:10] < 0.05)
    null_hits = int((res["p_fwe"][10:] < 0.05).sum())
    print(f"recorded: {null_hits} of 190 null voxels under p_fwe 0.05; {(res['p_unc'][10:] < 0.05).sum()} under p_unc 0.05")
    assert null_hits == PLANTED_NULL_UNDER_005
    assert np.all(res["p_fwe"] >= res["p_unc"]) and res["n_invalid"] == 0


# ------------------------------------------------------------------ invalid voxels in the restatement
def test_invalid_voxels_are_nan_and_enter_no_maximum():
    X = R.integer_case(6, 12, 5)
    X[:, 3] = 0.0
    X[:, 4] = 3.0
    X[2, 5] = np.nan
    mask = np.ones(12, bool)
    mask[7] = False
    res = R.run(X, exact=True, mask=mask)
    bad = np.zeros(12, bool)
    bad[[3, 5, 7]] = True
    assert np.array_equal(np.isnan(res["t"]), bad) and np.array_equal(np.isnan(res["p_unc"]), bad) and np.array_equal(np.isnan(res["p_fwe"]), bad)
    assert res["n_invalid"] == 3 and np.isposinf(res["t"][4]) and np.all(res["c"][bad] == 0)
    keep = ~bad
    alone = R.run(X[:, keep], exact=True)
    for key in ("max_stat", "max_t", "critical_t"):
        assert np.array_equal(res[key], alone[key])
    for key in ("count_unc", "count_fwe"):
        assert np.array_equal(res[key][keep], alone[key])
    two = R.run(X, kind=R.TWO, labels=np.array([1, 0, 1, 0, 0, 1]), R=20, mask=mask)
    assert np.isnan(two["t"][4]) and two["n_invalid"] == 4      # a constant voxel has no within-group variance


# ------------------------------------------------------------------ the premise of the float-input GPU case
def test_float_case_has_no_comparison_within_twice_the_fp32_bound():
    X = R.float_case()
    res64 = R.run(X, R=R.FLOAT_CASE["R"], seed=R.FLOAT_CASE["seed"], dtype=np.float64)
    margin, bound = R.near_tie_margin(X, res64)
    print(f"float case: smallest distance of a comparison {margin:.2f} bounds; largest bound {bound:.3e}")
    assert margin > 2.0
    res32 = R.run(X, R=R.FLOAT_CASE["R"], seed=R.FLOAT_CASE["seed"])
    assert np.array_equal(res32["count_unc"], res64["count_unc"]) and np.array_equal(res32["count_fwe"], res64["count_fwe"])


# ------------------------------------------------------------------ the binding, the refusals
NEW_SYMBOLS = ("nv_perm_splits", "nv_perm_workspace_bytes", "nv_perm_rank", "nv_perm_design", "nv_perm_stats", "nv_perm_maxstat", "nv_perm_finish")


def test_entry_points_are_declared_bound_and_listed_in_the_makefile():
    from neurovit_amd import _cabi
    for name in NEW_SYMBOLS:
        assert name in _cabi.lib.protos, name
        assert hasattr(_cabi.lib.load(), name), name
    assert _cabi.lib.protos["nv_perm_workspace_bytes"][0] is ctypes.c_long
    header = open(_cabi.HEADER).read()
    assert re.search(r"#define\s+NV_ABI_VERSION\s+8\b", header)      # new symbols within revision 8
    for name, value in (("NV_PERM_MAX_N", _cabi.PERM_MAX_N), ("NV_PERM_MAX_SPLITS", _cabi.PERM_MAX_SPLITS), ("NV_PERM_MAX_ALPHAS", _cabi.PERM_MAX_ALPHAS),
                        ("NV_PERM_TILE_V", _cabi.PERM_TILE_V), ("NV_PERM_TILE_R", _cabi.PERM_TILE_R), ("NV_PERM_TWO_SAMPLE", _cabi.PERM_KINDS["two_sample"]),
                        ("NV_PERM_TAIL_GREATER", _cabi.PERM_TAILS["greater"]), ("NV_PERM_TAIL_LESS", _cabi.PERM_TAILS["less"])):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name
    assert "#define NV_PERM_MAX_R (1 << 20)" in header and _cabi.PERM_MAX_R == 1 << 20
    assert f"0x{R.D1:X}" in header and f"0x{R.D2:X}" in header      # the hash domains are part of the contract
    mk = open(os.path.join(ROOT, "neurovit_amd", "csrc", "Makefile")).read()
    assert "perm_test.hip" in mk.split("SRCS")[1].split("\n")[0]
    import neurovit_amd
    from neurovit_amd import stats
    assert neurovit_amd.permutation_test is stats.permutation_test


def test_host_side_refusals_and_sizing_need_no_device():
    from neurovit_amd._cabi import last_error, lib
    buf, ibuf = (ctypes.c_float * 256)(), (ctypes.c_int * 64)()
    base = ctypes.addressof(buf)
    p = base + (-base % 16)
    ip = ctypes.addressof(ibuf)
    al = (ctypes.c_double * 2)(0.05, 0.01)
    alp = ctypes.cast(al, ctypes.c_void_p)
    assert lib.nv_perm_design(0, 1, 0, None, 16, 0, 1, p, None) != 0 and "N=1" in last_error()
    assert lib.nv_perm_design(0, 257, 0, None, 16, 0, 1, p, None) != 0 and "N=257" in last_error()
    assert lib.nv_perm_design(1, 2, 1, ip, 16, 0, 1, p, None) != 0 and "N=2" in last_error()
    assert lib.nv_perm_design(1, 7, 0, ip, 16, 0, 1, p, None) != 0 and "non-empty" in last_error()
    assert lib.nv_perm_design(0, 8, 0, None, (1 << 20) + 1, 0, 1, p, None) != 0 and "R=" in last_error()
    assert lib.nv_perm_design(0, 21, 0, None, 1 << 20, 1, 1, p, None) != 0 and "2^21" in last_error()
    assert lib.nv_perm_design(1, 7, 3, ip, 128, 1, 1, p, None) != 0 and "one-sample" in last_error()
    assert lib.nv_perm_stats(p, 7, 5, 8, 0, 0, None, None, p, p, p, ip, p, 256, None) != 0 and "ldx=7" in last_error()
    assert lib.nv_perm_maxstat(p, 7, 5, 8, p, 32, p, p, 0, 0, p, 1024, None) != 0 and "ldx=7" in last_error()
    assert lib.nv_perm_maxstat(p, 8, 5, 8, p, 32, p, p, 3, 0, p, 1024, None) != 0 and "tail" in last_error()
    assert lib.nv_perm_maxstat(p, 8, 5, 8, p, 32, p, p, 0, 257, p, 1024, None) != 0 and "splits" in last_error()
    assert lib.nv_perm_maxstat(p, 8, 5, 8, p, 32, p, p, 0, 0, p, 16, None) != 0 and "workspace" in last_error()
    assert lib.nv_perm_finish(0, 5, 32, 8, 0, p, alp, 9, p, p, ip, ip, p, p, p, p, 1024, None) != 0 and "n_alphas" in last_error()
    assert lib.nv_perm_finish(0, 5, 32, 8, 0, p, alp, 2, p, p, ip, ip, p, p, p, p, 16, None) != 0 and "workspace" in last_error()
    assert lib.nv_perm_splits(10000, 1000, 0) == 53 and lib.nv_perm_splits(10000, 729000, 0) == 1 and lib.nv_perm_splits(0, 10, 0) == 0
    assert lib.nv_perm_workspace_bytes(32, 130, 1) == 4 * (4 + 132 + 132 + 96) and lib.nv_perm_workspace_bytes(32, 130, 300) == 0
    for al_, rows in ((0.05, 100), (0.01, 100), (0.05, 32), (0.29, 100), (0.05, 131072)):
        assert lib.nv_perm_rank(al_, rows) == R.rank_of(al_, rows)


def test_host_check_program_is_clean_under_the_host_sanitizers():
    """tools/perm_test_host_check.cpp: the new host entry points (argument checks, sizing) in a stand-alone program built with
    -Xarch_host -fsanitize=address,undefined; it makes bad-argument calls only, so nothing is launched.  Nothing loaded into Python is sanitised."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "neurovit_amd", "csrc"), "perm-test-host-check"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    both = out.stdout + out.stderr
    assert "perm_test_host_check: ok" in out.stdout and "runtime error" not in both and "AddressSanitizer" not in both


def test_python_refusals_without_a_device():
    from neurovit_amd.stats import permutation_test
    x = torch.zeros(6, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        permutation_test(x)
    for bad in (dict(maps=x.double()), dict(maps=torch.zeros(6)), dict(maps=x, tail="both"), dict(maps=x, alphas=(0.0,)), dict(maps=x, alphas=(1.0,)),
                dict(maps=x, alphas=[0.1] * 9), dict(maps=x, splits=257), dict(maps=x, splits=-1), dict(maps=x, permutations=(1 << 20) + 1, exact=False),
                dict(maps=x, permutations=0, exact=False), dict(maps=x[:1]), dict(maps=torch.zeros(257, 4)), dict(maps=torch.zeros(21, 4), exact=True),
                dict(maps=x, mask=torch.ones(4, 4, dtype=torch.bool)), dict(maps=x, mask=torch.ones(4, 4, 4)),
                dict(maps=x, labels=[0, 1, 0, 1, 0]), dict(maps=x, labels=[0, 1, 2, 1, 0, 0]), dict(maps=x, labels=[0.0, 1.0, 0.0, 1.0, 0.0, 1.0]),
                dict(maps=x, labels=[0] * 6), dict(maps=x, labels=[1] * 6), dict(maps=x[:2], labels=[0, 1]), dict(maps=x, labels=[0, 1, 0, 1, 0, 1], exact=True),
                dict(maps=x, subjects=[0, 0, 1, 1, 3, 3]), dict(maps=x, subjects=[0, 0, 1, 1]), dict(maps=x, subjects=[0] * 6)):
        with pytest.raises(ValueError):
            permutation_test(**bad)
    with pytest.raises(ValueError, match="mixed labels"):
        permutation_test(x, labels=[0, 1, 1, 1, 0, 0], subjects=[0, 0, 1, 1, 2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a consistent labelling passes the host checks
        permutation_test(x, labels=[0, 0, 1, 1, 0, 0], subjects=[0, 0, 1, 1, 2, 2])
