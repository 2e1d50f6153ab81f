"""A numpy restatement of the permutation tests of csrc/perm_test.hip (include/neurovit_hip.h states the definitions): the same row rules,
the same fp32 a, c and u, the same ties.  tests/test_perm_test_cpu.py proves it against scipy and plain loops; tests/test_perm_test_gpu.py
holds the kernels to it.

The facts it rests on.  ONE SAMPLE, sign flips m_i = +-1: Q = sum x_i^2 does not change under a flip; with S = sum m_i x_i the flipped sample
has mean S / N and variance (Q - S^2 / N) / (N - 1), so t = (S / N) / sqrt((Q - S^2 / N) / (N (N - 1))) = u sqrt((N - 1) / (1 - u^2)) with
u = S / sqrt(N Q), |u| <= 1 by Cauchy-Schwarz.  TWO SAMPLES, marks m_i in {0, 1} with n_A ones: T = sum x_i and SS = Q - T^2 / N do not
change under a relabelling; with S = sum m_i x_i the difference of the group means is (S - n_A T / N) N / (n_A n_B), the pooled within-group
sum of squares is SS - (S - n_A T / N)^2 N / (n_A n_B), and Student's t becomes u sqrt((N - 2) / (1 - u^2)) with
u = (S - n_A T / N) / sqrt(n_A n_B SS / N).  d t / d u = sqrt(df) (1 - u^2)^(-3/2) > 0: t is strictly increasing in u, so maxima, ties and
counts may be taken on u."""
import numpy as np

MASK64 = (1 << 64) - 1
D1, D2 = 0x5045524D31, 0x5045524D32      # the hash domains of the sign flips and of the two-sample sort keys
ONE, TWO = "one_sample", "two_sample"


def hash64(seed, grp):
    """nv_hash64 (csrc/common.h) on Python integers"""
    x = (((grp + 0x9E3779B97F4A7C15) & MASK64) * 0xBF58476D1CE4E5B9 & MASK64) ^ (seed & MASK64)
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & MASK64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & MASK64
    x ^= x >> 31
    return x


def npad(N):
    return (N + 3) & ~3


def design(kind, N, R, seed=0, exact=False, labels=None):
    """M fp32 [R, Npad]: row 0 the observed labelling, then the three row rules"""
    M = np.zeros((R, npad(N)), np.float32)
    if kind == ONE:
        M[:, :N] = 1.0
        words = (N + 63) // 64
        for r in range(1, R):
            for i in range(N):
                if exact:
                    neg = (r >> i) & 1
                else:
                    neg = (hash64(seed ^ D1, r * words + (i >> 6)) >> (i & 63)) & 1
                if neg:
                    M[r, i] = -1.0
        return M
    labels = np.asarray(labels)
    n_a = int((labels == 1).sum())
    M[0, :N] = labels == 1
    for r in range(1, R):
        keys = [hash64(seed ^ D2, r * N + i) for i in range(N)]
        order = sorted(range(N), key=lambda i: (keys[i], i))      # ascending keys, equal keys to the lower index
        M[r, order[:n_a]] = 1.0
    return M


def t_of_u(u, df):
    u = np.asarray(u, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        uu = u * u
        return u * np.sqrt(df / (1.0 - uu))


def degrees(kind, N):
    return float(N - 1 if kind == ONE else N - 2)


def stats(X, kind, labels=None, mask=None):
    """The per-voxel constants of X fp32 [N, V]: sums in double over the subjects in ascending order, a and c rounded to fp32 once.
    -> dict(a, c fp32; t fp32 (NaN where invalid); valid bool; n_invalid; u0 float64)"""
    X = np.asarray(X, np.float32)
    N, V = X.shape
    T, Q, SA = np.zeros(V), np.zeros(V), np.zeros(V)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(N):
            d = X[i].astype(np.float64)
            T = T + d
            Q = Q + d * d
            if kind == TWO and labels[i] == 1:
                SA = SA + d
        ok = np.isfinite(X).all(0)
        if mask is not None:
            ok &= np.asarray(mask, bool).reshape(V)
        if kind == ONE:
            ok &= Q > 0.0
            root = np.sqrt(float(N) * Q)
            aD = np.zeros(V)
            u0 = T / root
            u0 = np.where(X.min(0) == X.max(0), np.where(T > 0.0, 1.0, -1.0), u0)
        else:
            n_a = int((np.asarray(labels) == 1).sum())
            SS = Q - (T * T) / float(N)
            ok &= SS > 0.0
            aD = (float(n_a) * T) / float(N)
            root = np.sqrt(((float(n_a) * float(N - n_a)) * SS) / float(N))
            u0 = (SA - aD) / root
        cf, af = (1.0 / root).astype(np.float32), aD.astype(np.float32)
        ok &= (cf > 0) & np.isfinite(cf) & np.isfinite(af)
        t = t_of_u(np.clip(u0, -1.0, 1.0), degrees(kind, N)).astype(np.float32)
    return dict(a=np.where(ok, af, np.float32(0)).astype(np.float32), c=np.where(ok, cf, np.float32(0)).astype(np.float32),
                t=np.where(ok, t, np.float32("nan")).astype(np.float32), valid=ok, n_invalid=int((~ok).sum()), u0=u0)


def statistic(X, M, a, c, tail, dtype=np.float32):
    """stat [R, V]: S = M X (float64: exact for the integer inputs; the float64 restatement otherwise), then u = (S - a) c with every operation
    rounded to `dtype`, clamped to [-1, 1]; |u|, u or -u"""
    N = X.shape[0]
    S = (M[:, :N].astype(np.float64) @ X.astype(np.float64)).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((S - a.astype(dtype)[None, :]).astype(dtype) * c.astype(dtype)[None, :]).astype(dtype)
    u = np.clip(u, dtype(-1), dtype(1))
    return np.abs(u) if tail == "two" else (u if tail == "greater" else -u)


def rank_of(alpha, R):
    """nv_perm_rank: k = R - floor(alpha R + 1e-9) = ceil((1 - alpha) R) without the rounding of 1 - alpha"""
    return R - int(np.floor(alpha * float(R) + 1e-9))


def finish(stat, valid, kind, N, alphas=()):
    """the reductions of stat [R, V] (row 0 observed): row maxima over the valid voxels, counts with >=, p = float32(count / R), the null
    distribution and the critical values in t units"""
    R, V = stat.shape
    df = degrees(kind, N)
    if valid.any():
        max_stat = stat[:, valid].max(1) + stat.dtype.type(0)
    else:
        max_stat = np.full(R, -np.inf, stat.dtype)
    count_unc = np.where(valid, (stat >= stat[0][None, :]).sum(0), 0).astype(np.int32)
    count_fwe = np.where(valid, (max_stat[:, None] >= stat[0][None, :]).sum(0), 0).astype(np.int32)
    with np.errstate(invalid="ignore"):
        p_unc = np.where(valid, (count_unc / float(R)).astype(np.float32), np.float32("nan")).astype(np.float32)
        p_fwe = np.where(valid, (count_fwe / float(R)).astype(np.float32), np.float32("nan")).astype(np.float32)
    max_t = t_of_u(np.clip(max_stat.astype(np.float64), -1.0, 1.0), df).astype(np.float32)
    srt = np.sort(max_stat)
    crit = np.array([t_of_u(np.clip(np.float64(srt[rank_of(al, R) - 1]), -1.0, 1.0), df) for al in alphas], np.float64).astype(np.float32)
    return dict(max_stat=max_stat, count_unc=count_unc, count_fwe=count_fwe, p_unc=p_unc, p_fwe=p_fwe, max_t=max_t, critical_t=crit)


def run(X, kind=ONE, labels=None, R=None, tail="two", mask=None, seed=0, exact=False, alphas=(0.05, 0.01), dtype=np.float32):
    """the whole test: design, constants, statistic, reductions"""
    X = np.asarray(X, np.float32)
    N = X.shape[0]
    R = (1 << N) if exact else R
    M = design(kind, N, R, seed, exact, labels)
    st = stats(X, kind, labels, mask)
    Xz = np.where(st["valid"][None, :], X, np.float32(0))      # an invalid voxel carries zeros (and its c is 0)
    stat = statistic(Xz, M, st["a"], st["c"], tail, dtype)
    out = finish(stat, st["valid"], kind, N, alphas)
    out.update(M=M, stat=stat, **st)
    return out


def accumulation_bound(X, c):
    """the first-order bound of the fp32 error of u per voxel: (N + 2) 2^-24 sum_i |x_i| c(v) - N - 1 roundings of the accumulated sum, one of the
    subtraction, one of the product, each at most 2^-24 of a magnitude below sum |x_i| (two samples: |S - a| <= sum |x_i| as well)"""
    N = X.shape[0]
    return (N + 2) * 2.0 ** -24 * np.abs(X.astype(np.float64)).sum(0) * c.astype(np.float64)


def near_tie_margin(X, res64):
    """min over the rows r >= 1 and the valid voxels of |stat_r(v) - stat_0(v)| / bound(v) and of |max_r - stat_0(v)| / max bound, on the float64
    restatement res64 = run(..., dtype=np.float64): above 2, no comparison of the fp32 kernel can fall on the other side"""
    valid = res64["valid"]
    Xz = np.where(valid[None, :], X, np.float32(0))
    bound = accumulation_bound(Xz, res64["c"])[valid]
    stat = res64["stat"][:, valid]
    cell = (np.abs(stat[1:] - stat[0][None, :]) / bound[None, :]).min()
    row = (np.abs(res64["max_stat"][1:, None] - stat[0][None, :]) / bound.max()).min()
    return float(min(cell, row)), float(bound.max())


# ------------------------------------------------------------------ the cases of the GPU test (the CPU test proves their premises)
def integer_case(N, V, seed, kind=ONE):
    """small integers: every sum of the test is exact in fp32, whatever its order"""
    rng = np.random.default_rng(seed)
    X = rng.integers(-4, 5, size=(N, V)).astype(np.float32)
    X[:, 0] += 2.0      # one voxel with an effect
    return X


FLOAT_CASE = dict(N=10, V=130, R=200, data_seed=3, seed=1)      # randn; the seeds are those for which near_tie_margin > 2 (asserted in the CPU test)


def float_case():
    rng = np.random.default_rng(FLOAT_CASE["data_seed"])
    X = rng.standard_normal((FLOAT_CASE["N"], FLOAT_CASE["V"])).astype(np.float32)
    X[:, :5] += 1.0
    return X
