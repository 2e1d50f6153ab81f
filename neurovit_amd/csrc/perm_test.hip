// Group-level permutation tests with the maximum statistic: the design matrix (nv_perm_design), the per-voxel constants and the observed t
// (nv_perm_stats), the fused product + two-way reduction over all permutations (nv_perm_maxstat) and the p-value maps, the null distribution
// and the critical values (nv_perm_finish).  The definitions are in the header.  Nothing here reads back, nothing uses atomics; every
// floating-point sum has one fixed order and every count is an integer, so the bits do not depend on the grid, the split count or the CU count.
#include <math.h>

#include "eval_common.h"

#pragma clang fp contract(off)

namespace {

constexpr uint64_t PERM_D1 = 0x5045524D31ull;      // "PERM1": the sign flips of the one-sample test (ABI: the header states the draw rule)
constexpr uint64_t PERM_D2 = 0x5045524D32ull;      // "PERM2": the sort keys of the two-sample labellings
constexpr int TV = NV_PERM_TILE_V, TR = NV_PERM_TILE_R;
constexpr int FIN_THREADS = 1024, FIN_CHUNK = 4096;

// every operation rounded on its own (the pragma above; rsub and rmul of eval_common.h): the numpy restatement repeats these expressions
__device__ __forceinline__ double clamp1(double u) { return u > 1.0 ? 1.0 : (u < -1.0 ? -1.0 : u); }
// t = u sqrt(df / (1 - u^2)), strictly increasing on [-1, 1]; +-inf at the ends
__device__ __forceinline__ double t_of_u(double u, double df) {
  const double uu = u * u;
  const double den = 1.0 - uu;
  return u * sqrt(df / den);
}
template <int TAIL>
__device__ __forceinline__ float stat_of(float acc, float a, float c) {
  float u = rmul(rsub(acc, a), c);
  u = fminf(fmaxf(u, -1.f), 1.f);
  return TAIL == NV_PERM_TAIL_TWO ? fabsf(u) : (TAIL == NV_PERM_TAIL_GREATER ? u : -u);
}

// ------------------------------------------------------------------------------------------------ design
// One sample: one thread per cell of M [R, Npad].
__global__ __launch_bounds__(256) void perm_design_one_kernel(int N, int Npad, int R, int exact, unsigned long long seed, float* __restrict__ M) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)R * Npad) return;
  const int r = (int)(e / Npad), i = (int)(e - (long)r * Npad);
  float v = 0.f;
  if (i < N) {
    bool neg = false;
    if (r > 0) {
      if (exact) neg = (((unsigned)r >> i) & 1u) != 0u;      // exact: N <= 20, so i < 32
      else {
        const unsigned long long words = (unsigned long long)((N + 63) >> 6);
        const uint64_t h = nv_hash64(seed ^ PERM_D1, (unsigned long long)r * words + (unsigned long long)(i >> 6));
        neg = ((h >> (i & 63)) & 1ull) != 0ull;
      }
    }
    v = neg ? -1.f : 1.f;
  }
  M[e] = v;
}

// Two samples: one workgroup per row.  Row 0 is the given labelling; row r >= 1 puts the n_a subjects with the smallest keys into group A
// (equal keys: the lower index first).
__global__ __launch_bounds__(256) void perm_design_two_kernel(int N, int Npad, int n_a, const int* __restrict__ labels, unsigned long long seed,
                                                              float* __restrict__ M) {
  __shared__ uint64_t keys[NV_PERM_MAX_N];
  const int r = blockIdx.x, i = threadIdx.x;
  float* row = M + (long)r * Npad;
  if (r == 0) {
    if (i < Npad) row[i] = (i < N && labels[i] == 1) ? 1.f : 0.f;
    return;
  }
  if (i < N) keys[i] = nv_hash64(seed ^ PERM_D2, (unsigned long long)r * (unsigned long long)N + (unsigned long long)i);
  __syncthreads();
  if (i >= Npad) return;
  float v = 0.f;
  if (i < N) {
    const uint64_t mine = keys[i];
    int rank = 0;
    for (int j = 0; j < N; ++j) rank += (keys[j] < mine) || (keys[j] == mine && j < i);
    v = rank < n_a ? 1.f : 0.f;
  }
  row[i] = v;
}

// ------------------------------------------------------------------------------------------------ per-voxel constants
// One thread per voxel: T, Q (and the sum over group A) in double, ascending subject order, products and sums rounded on their own.
__global__ __launch_bounds__(256) void perm_stats_kernel(const float* __restrict__ X, long ldx, int N, int V, int kind, int n_a, const int* __restrict__ labels,
                                                         const unsigned char* __restrict__ mask, float* __restrict__ av, float* __restrict__ cv,
                                                         float* __restrict__ tv, int* __restrict__ inval_part) {
  __shared__ int red[1][4];
  const int tid = threadIdx.x;
  const int v = blockIdx.x * 256 + tid;
  int bad = 0;
  if (v < V) {
    bool ok = !mask || mask[v] != 0;
    double T = 0.0, Q = 0.0, SA = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < N; ++i) {
      const float x = X[(long)i * ldx + v];
      ok = ok && __builtin_isfinite(x);
      const double d = (double)x;
      const double dd = d * d;
      T = T + d;
      Q = Q + dd;
      if (kind == NV_PERM_TWO_SAMPLE && labels[i] == 1) SA = SA + d;
      mn = fminf(mn, x);
      mx = fmaxf(mx, x);
    }
    double root, aD = 0.0, u0, df;
    if (kind == NV_PERM_ONE_SAMPLE) {
      ok = ok && Q > 0.0;
      root = sqrt((double)N * Q);
      u0 = T / root;
      if (mn == mx) u0 = T > 0.0 ? 1.0 : -1.0;      // all values equal (and not zero: Q > 0): |u| = 1 whatever the rounding of T and Q
      df = (double)(N - 1);
    } else {
      const double SS = Q - (T * T) / (double)N;
      ok = ok && SS > 0.0;
      aD = ((double)n_a * T) / (double)N;
      root = sqrt((((double)n_a * (double)(N - n_a)) * SS) / (double)N);
      u0 = (SA - aD) / root;
      df = (double)(N - 2);
    }
    const float cf = (float)(1.0 / root), af = (float)aD;
    ok = ok && cf > 0.f && __builtin_isfinite(cf) && __builtin_isfinite(af);
    av[v] = ok ? af : 0.f;
    cv[v] = ok ? cf : 0.f;
    tv[v] = ok ? (float)t_of_u(clamp1(u0), df) : __builtin_nanf("");
    bad = ok ? 0 : 1;
  }
  bad = block_sum4(bad, red);
  if (tid == 0) inval_part[blockIdx.x] = bad;
}

__global__ __launch_bounds__(256) void perm_invalid_sum_kernel(const int* __restrict__ part, int n, int* __restrict__ out) {
  __shared__ int red[1][4];
  int s = 0;
  for (int b = threadIdx.x; b < n; b += 256) s += part[b];
  s = block_sum4(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ------------------------------------------------------------------------------------------------ the hot path
// Workgroup (x, y) = 4 waves: the TV = 64 voxels v0 = 64 x .. of the maps against the rows [rb, re) of M (split y).  The [Npad, 64] slab of X
// is staged in LDS once (invalid voxels, columns past V and rows past N as zeros); slab row k keeps its 16-column groups XOR-ed with
// key(k) = ((k >> 2) ^ k) & 3, so that the four lane groups of an MFMA operand read - rows k0 + 4 g + t or k0 + 4 t + g - fall on 64 different
// banks.  Wave w walks the row tiles r0 = rb + 16 w, + 64, ...: a 16-row x 64-voxel block of P = M X^T-slab in four accumulators
// (lane (i, g), register r of block nb = P[r0 + 4 g + r][v0 + 16 nb + i]), the rows of M straight from L2 - 16 bytes per lane and 16 subjects,
// the last Npad % 16 subjects four at a time.  The epilogue forms the statistic, counts it against the voxel's own row-0 value (computed by
// every wave through the same product, so the same bits) and reduces the row maxima over the 16 lanes of a group.
__device__ __forceinline__ int slab_key(int k) { return ((k >> 2) ^ k) & 3; }

__device__ __forceinline__ void perm_tile_product(const float* __restrict__ M, int Npad, int R, int r0, const float* slab, int i, int g, f32x4 (&acc)[4]) {
  const float* mrow = M + (long)min(r0 + i, R - 1) * Npad;      // (rows past R repeat the last row: they are never counted or written)
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  int kc = 0;
  for (; kc + 16 <= Npad; kc += 16) {
    const f32x4 af = *reinterpret_cast<const f32x4*>(mrow + kc + 4 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = kc + 4 * g + t;
      const float* srow = slab + k * TV + i;
      const int key = slab_key(k);
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma4(af[t], srow[16 * (nb ^ key)], acc[nb]);
    }
  }
  for (; kc < Npad; kc += 4) {
    const int k = kc + g;
    const float a = mrow[k];
    const float* srow = slab + k * TV + i;
    const int key = slab_key(k);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[nb] = mfma4(a, srow[16 * (nb ^ key)], acc[nb]);
  }
}

template <int TAIL>
__global__ __launch_bounds__(256) void perm_maxstat_kernel(const float* __restrict__ X, long ldx, int N, int Npad, int V, const float* __restrict__ M, int R,
                                                           const float* __restrict__ av, const float* __restrict__ cv, int rows_per_split, int nvt,
                                                           float* __restrict__ stat0, unsigned* __restrict__ cnt_part, float* __restrict__ pmax) {
  extern __shared__ __attribute__((aligned(16))) float psm[];      // [Npad][TV] slab | unsigned [4][TV]
  float* slab = psm;
  unsigned* red = reinterpret_cast<unsigned*>(psm + Npad * TV);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
  const int v0 = blockIdx.x * TV;
  const int rb = blockIdx.y * rows_per_split, re = min(rb + rows_per_split, R);
  {
    const int v = v0 + lane;
    const bool ok = v < V && cv[v] > 0.f;
    for (int k = wid; k < Npad; k += 4) slab[k * TV + (lane ^ (16 * slab_key(k)))] = (ok && k < N) ? X[(long)k * ldx + v] : 0.f;
  }
  float ca[4], cc[4], s0[4];
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    const int v = v0 + 16 * nb + i;
    ca[nb] = v < V ? av[v] : 0.f;
    cc[nb] = v < V ? cv[v] : 0.f;
  }
  __syncthreads();
  f32x4 acc[4];
  perm_tile_product(M, Npad, R, 0, slab, i, g, acc);
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    s0[nb] = __shfl(stat_of<TAIL>(acc[nb][0], ca[nb], cc[nb]), i, 64);      // row 0 lives in register 0 of the lanes g = 0
    if (blockIdx.y == 0 && wid == 0 && g == 0 && v0 + 16 * nb + i < V) stat0[v0 + 16 * nb + i] = s0[nb];
  }
  unsigned cnt[4] = {0u, 0u, 0u, 0u};
  for (int r0 = rb + 16 * wid; r0 < re; r0 += TR) {
    perm_tile_product(M, Npad, R, r0, slab, i, g, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + 4 * g + r;
      const bool rok = row < re;
      float m = -INFINITY;
#pragma unroll
      for (int nb = 0; nb < 4; ++nb) {
        const float s = stat_of<TAIL>(acc[nb][r], ca[nb], cc[nb]);
        const bool valid = cc[nb] > 0.f;
        cnt[nb] += (unsigned)(rok && valid && s >= s0[nb]);
        m = valid ? fmaxf(m, s) : m;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
      if (i == 0 && rok) pmax[(long)row * nvt + blockIdx.x] = m;
    }
  }
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    cnt[nb] += __shfl_xor(cnt[nb], 16, 64);
    cnt[nb] += __shfl_xor(cnt[nb], 32, 64);
    if (g == 0) red[wid * TV + 16 * nb + i] = cnt[nb];
  }
  __syncthreads();
  if (tid < TV && v0 + tid < V) cnt_part[(long)blockIdx.y * V + v0 + tid] = (red[tid] + red[TV + tid]) + (red[2 * TV + tid] + red[3 * TV + tid]);
}

// ------------------------------------------------------------------------------------------------ finish
// First launch: one wave per row, the maximum over the row's voxel tiles (order-independent, so exact); -0 becomes +0.
__global__ __launch_bounds__(256) void perm_rowmax_kernel(const float* __restrict__ pmax, int R, int nvt, double df, float* __restrict__ max_stat,
                                                          float* __restrict__ max_t) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;
  float m = -INFINITY;
  for (int t = lane; t < nvt; t += 64) m = fmaxf(m, pmax[(long)r * nvt + t]);
  m = wave_max(m) + 0.f;
  if (lane == 0) {
    max_stat[r] = m;
    max_t[r] = (float)t_of_u(clamp1((double)m), df);
  }
}

// ascending fp32 order as ascending unsigned order
__device__ __forceinline__ unsigned key_of_float(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float float_of_key(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct PermRanks {
  int n;
  int k[NV_PERM_MAX_ALPHAS];
};

// Second launch.  Workgroups 0 .. nvb - 1: one voxel per thread - the split partials of count_unc added in split order, count_fwe by comparing
// the voxel's observed statistic with all R maxima (they go through LDS in chunks, every lane reads the same address), both p-values.  The
// last workgroup: the critical values, the k-th smallest maximum by a bitwise search over the ordered keys - 32 counting passes over the R maxima.
__global__ __launch_bounds__(FIN_THREADS) void perm_pvalue_kernel(const float* __restrict__ max_stat, int R, int V, int S, const float* __restrict__ cv,
                                                                  const float* __restrict__ stat0, const unsigned* __restrict__ cnt_part, double df,
                                                                  PermRanks ranks, int* __restrict__ count_unc, int* __restrict__ count_fwe,
                                                                  float* __restrict__ p_unc, float* __restrict__ p_fwe, float* __restrict__ critical_t) {
  __shared__ __attribute__((aligned(16))) float chunk[FIN_CHUNK];
  __shared__ int red[FIN_THREADS / 64][NV_PERM_MAX_ALPHAS];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nvb = gridDim.x - 1;
  if ((int)blockIdx.x < nvb) {
    const int v = blockIdx.x * FIN_THREADS + tid;
    const bool valid = v < V && cv[v] > 0.f;
    const float s0 = valid ? stat0[v] : INFINITY;
    unsigned cu = 0u, cf = 0u;
    if (valid)
      for (int s = 0; s < S; ++s) cu += cnt_part[(long)s * V + v];
    for (int c0 = 0; c0 < R; c0 += FIN_CHUNK) {
      for (int e = tid; e < FIN_CHUNK; e += FIN_THREADS) chunk[e] = c0 + e < R ? max_stat[c0 + e] : -INFINITY;
      __syncthreads();
      const int n = min(FIN_CHUNK, R - c0);
      for (int e = 0; e < n; e += 4) {      // (the pad of the last quad is -inf: it never reaches a finite s0)
        const f32x4 m = *reinterpret_cast<const f32x4*>(chunk + e);
        cf += (unsigned)(m[0] >= s0) + (unsigned)(m[1] >= s0) + (unsigned)(m[2] >= s0) + (unsigned)(m[3] >= s0);
      }
      __syncthreads();
    }
    if (v < V) {
      count_unc[v] = valid ? (int)cu : 0;
      count_fwe[v] = valid ? (int)cf : 0;
      p_unc[v] = valid ? (float)((double)cu / (double)R) : __builtin_nanf("");
      p_fwe[v] = valid ? (float)((double)cf / (double)R) : __builtin_nanf("");
    }
    return;
  }
  unsigned ans[NV_PERM_MAX_ALPHAS];
#pragma unroll
  for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) ans[j] = 0u;
  for (int bit = 31; bit >= 0; --bit) {
    int below[NV_PERM_MAX_ALPHAS];
#pragma unroll
    for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) below[j] = 0;
    for (int r = tid; r < R; r += FIN_THREADS) {
      const unsigned key = key_of_float(max_stat[r]);
#pragma unroll
      for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j)
        if (j < ranks.n) below[j] += (int)(key < (ans[j] | (1u << bit)));
    }
#pragma unroll
    for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) {
      if (j >= ranks.n) continue;      // (uniform: the alphas in use)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) below[j] += __shfl_xor(below[j], o, 64);
      if (lane == 0) red[wid][j] = below[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) {
      if (j >= ranks.n) continue;
      int total = 0;
      for (int w = 0; w < FIN_THREADS / 64; ++w) total += red[w][j];
      if (total < ranks.k[j]) ans[j] |= 1u << bit;      // fewer than k keys lie below the trial value: the k-th smallest is at least that large
    }
    __syncthreads();
  }
  if (tid < ranks.n) {
    unsigned mine = 0u;
#pragma unroll
    for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) mine = tid == j ? ans[j] : mine;
    critical_t[tid] = (float)t_of_u(clamp1((double)float_of_key(mine)), df);
  }
}

inline int perm_npad(int N) { return (N + 3) & ~3; }
inline int perm_vtiles(int V) { return (V + TV - 1) / TV; }

int perm_resolve_splits(int R, int V, int splits) { return nv_resolve_splits(perm_vtiles(V), (R + TR - 1) / TR, splits, NV_PERM_MAX_SPLITS); }

bool perm_shape_ok(int R, int V, int splits) { return R >= 1 && R <= NV_PERM_MAX_R && V >= 1 && splits >= 0 && splits <= NV_PERM_MAX_SPLITS; }

// the workspace, in 4-byte words: the invalid counts of nv_perm_stats' workgroups | stat0 [V] | the count partials [S][V] | the row maxima [R][nvt]
struct PermWs {
  long inval, stat0, cnt, pmax, words;
};
PermWs perm_ws(int R, int V, int S) {
  auto up4 = [](long n) { return (n + 3) & ~3L; };
  PermWs w;
  w.inval = 0;
  w.stat0 = up4((V + 255) / 256);
  w.cnt = w.stat0 + up4(V);
  w.pmax = w.cnt + up4((long)S * V);
  w.words = w.pmax + up4((long)R * perm_vtiles(V));
  return w;
}

int perm_check_design(const char* who, int kind, int N, int n_a) {
  NV_CHECK_ARG(kind == NV_PERM_ONE_SAMPLE || kind == NV_PERM_TWO_SAMPLE, "%s: unknown kind %d", who, kind);
  NV_CHECK_ARG(N >= 2 && N <= NV_PERM_MAX_N, "%s: N=%d outside [2, %d]", who, N, NV_PERM_MAX_N);
  NV_CHECK_ARG(kind != NV_PERM_TWO_SAMPLE || (N >= 3 && n_a >= 1 && n_a <= N - 1), "%s: two samples need N=%d >= 3 and both groups non-empty, got n_a=%d", who, N, n_a);
  return NV_OK;
}

}  // namespace

extern "C" int nv_perm_splits(int R, int V, int splits) { return perm_shape_ok(R, V, splits) ? perm_resolve_splits(R, V, splits) : 0; }

extern "C" long nv_perm_workspace_bytes(int R, int V, int splits) {
  const int s = nv_perm_splits(R, V, splits);
  if (s < 1) return 0;
  return perm_ws(R, V, s).words * 4L;
}

extern "C" int nv_perm_design(int kind, int N, int n_a, const int* labels, int R, int exact, unsigned long seed, float* M, void* stream) {
  if (int rc = perm_check_design("nv_perm_design", kind, N, n_a)) return rc;
  NV_CHECK_ARG(M && nv_aligned16(M), "nv_perm_design: M is NULL or not 16-byte aligned");
  NV_CHECK_ARG(R >= 1 && R <= NV_PERM_MAX_R, "nv_perm_design: R=%d outside [1, %d]", R, NV_PERM_MAX_R);
  NV_CHECK_ARG(kind != NV_PERM_TWO_SAMPLE || (labels && nv_aligned(labels, 4)), "nv_perm_design: two samples need the labels (int32 [N], 4-byte aligned)");
  if (exact) {
    NV_CHECK_ARG(kind == NV_PERM_ONE_SAMPLE, "nv_perm_design: exact enumeration exists for the one-sample sign flips only");
    NV_CHECK_ARG(N <= 20, "nv_perm_design: exact enumeration of 2^%d sign flips exceeds the %d rows of a call", N, NV_PERM_MAX_R);
    NV_CHECK_ARG(R == (1 << N), "nv_perm_design: exact enumeration of N=%d needs R = 2^N = %d rows, got %d", N, 1 << N, R);
  }
  const int Npad = perm_npad(N);
  hipStream_t s = (hipStream_t)stream;
  if (kind == NV_PERM_ONE_SAMPLE) {
    const long cells = (long)R * Npad;
    hipLaunchKernelGGL(perm_design_one_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, N, Npad, R, exact ? 1 : 0, (unsigned long long)seed, M);
  } else {
    hipLaunchKernelGGL(perm_design_two_kernel, dim3(R), dim3(256), 0, s, N, Npad, n_a, labels, (unsigned long long)seed, M);
  }
  NV_CHECK_LAUNCH("nv_perm_design");
  return NV_OK;
}

extern "C" int nv_perm_stats(const float* X, long ldx, int N, int V, int kind, int n_a, const int* labels, const unsigned char* mask, float* a, float* c,
                             float* t, int* n_invalid, void* workspace, long ws_bytes, void* stream) {
  if (int rc = perm_check_design("nv_perm_stats", kind, N, n_a)) return rc;
  NV_CHECK_ARG(X && a && c && t && n_invalid && workspace, "nv_perm_stats: null pointer");
  NV_CHECK_ARG(V >= 1 && ldx >= V, "nv_perm_stats: V=%d must be positive and ldx=%ld must cover it", V, ldx);
  NV_CHECK_ARG(kind != NV_PERM_TWO_SAMPLE || labels, "nv_perm_stats: two samples need the labels");
  NV_CHECK_ARG(nv_aligned(X, 4) && nv_aligned(a, 4) && nv_aligned(c, 4) && nv_aligned(t, 4) && nv_aligned(n_invalid, 4) && nv_aligned(labels, 4) && nv_aligned(workspace, 16),
               "nv_perm_stats: every array 4-byte aligned, the workspace 16-byte aligned");
  const int nb = (V + 255) / 256;
  NV_CHECK_ARG(ws_bytes >= 4L * nb, "nv_perm_stats: the workspace has %ld bytes, %ld needed (nv_perm_workspace_bytes)", ws_bytes, 4L * nb);
  hipStream_t s = (hipStream_t)stream;
  int* part = (int*)workspace;
  hipLaunchKernelGGL(perm_stats_kernel, dim3(nb), dim3(256), 0, s, X, ldx, N, V, kind, n_a, labels, mask, a, c, t, part);
  hipLaunchKernelGGL(perm_invalid_sum_kernel, dim3(1), dim3(256), 0, s, part, nb, n_invalid);
  NV_CHECK_LAUNCH("nv_perm_stats");
  return NV_OK;
}

extern "C" int nv_perm_maxstat(const float* X, long ldx, int N, int V, const float* M, int R, const float* a, const float* c, int tail, int splits,
                               void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(X && M && a && c && workspace, "nv_perm_maxstat: null pointer");
  NV_CHECK_ARG(N >= 2 && N <= NV_PERM_MAX_N, "nv_perm_maxstat: N=%d outside [2, %d]", N, NV_PERM_MAX_N);
  NV_CHECK_ARG(R >= 1 && R <= NV_PERM_MAX_R, "nv_perm_maxstat: R=%d outside [1, %d]", R, NV_PERM_MAX_R);
  NV_CHECK_ARG(V >= 1 && ldx >= V, "nv_perm_maxstat: V=%d must be positive and ldx=%ld must cover it", V, ldx);
  NV_CHECK_ARG(tail == NV_PERM_TAIL_TWO || tail == NV_PERM_TAIL_GREATER || tail == NV_PERM_TAIL_LESS, "nv_perm_maxstat: unknown tail %d", tail);
  NV_CHECK_ARG(splits >= 0 && splits <= NV_PERM_MAX_SPLITS, "nv_perm_maxstat: splits=%d outside [0, %d] (0 = automatic)", splits, NV_PERM_MAX_SPLITS);
  NV_CHECK_ARG(nv_aligned(X, 4) && nv_aligned16(M) && nv_aligned(a, 4) && nv_aligned(c, 4) && nv_aligned16(workspace),
               "nv_perm_maxstat: X, a and c 4-byte aligned, M and the workspace 16-byte aligned");
  const int S = perm_resolve_splits(R, V, splits);
  const PermWs w = perm_ws(R, V, S);
  NV_CHECK_ARG(ws_bytes >= w.words * 4L, "nv_perm_maxstat: %d splits need a workspace of %ld bytes (nv_perm_workspace_bytes), got %ld", S, w.words * 4L, ws_bytes);
  const int Npad = perm_npad(N), nvt = perm_vtiles(V), rtiles = (R + TR - 1) / TR, rps = ((rtiles + S - 1) / S) * TR;
  const size_t lds = (size_t)(Npad * TV + 4 * TV) * sizeof(float);
  static_assert((size_t)(NV_PERM_MAX_N * TV + 4 * TV) * sizeof(float) <= 80 * 1024, "two workgroups per CU at N = 256");
  static_assert(NV_PERM_MAX_SPLITS <= 65535 && TR == 64 && TV == 64, "the grid's y extent; 4 waves x 16 rows, 4 blocks x 16 voxels");
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  auto launch = [&](auto kernel) -> int {
    if (lds > 64 * 1024) {
      static bool allowed = false;      // (of this instantiation of the lambda: one per kernel)
      if (int rc = allow_lds(kernel, (NV_PERM_MAX_N * TV + 4 * TV) * (int)sizeof(float), allowed, "nv_perm_maxstat")) return rc;
    }
    hipLaunchKernelGGL(kernel, dim3(nvt, S), dim3(256), lds, s, X, ldx, N, Npad, V, M, R, a, c, rps, nvt, ws + w.stat0, (unsigned*)(ws + w.cnt), ws + w.pmax);
    return NV_OK;
  };
  const int rc = tail == NV_PERM_TAIL_TWO       ? launch(perm_maxstat_kernel<NV_PERM_TAIL_TWO>)
                 : tail == NV_PERM_TAIL_GREATER ? launch(perm_maxstat_kernel<NV_PERM_TAIL_GREATER>)
                                                : launch(perm_maxstat_kernel<NV_PERM_TAIL_LESS>);
  if (rc != NV_OK) return rc;
  NV_CHECK_LAUNCH("nv_perm_maxstat");
  return NV_OK;
}

extern "C" int nv_perm_rank(double alpha, int R) {
  if (!(alpha > 0.0 && alpha < 1.0) || R < 1) return 0;
  return R - (int)floor(alpha * (double)R + 1e-9);
}

extern "C" int nv_perm_finish(int kind, int N, int R, int V, int splits, const float* c, const double* alphas, int n_alphas, float* max_stat, float* max_t,
                              int* count_unc, int* count_fwe, float* p_unc, float* p_fwe, float* critical_t, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(kind == NV_PERM_ONE_SAMPLE || kind == NV_PERM_TWO_SAMPLE, "nv_perm_finish: unknown kind %d", kind);
  NV_CHECK_ARG(N >= (kind == NV_PERM_TWO_SAMPLE ? 3 : 2) && N <= NV_PERM_MAX_N, "nv_perm_finish: N=%d outside [%d, %d]", N, kind == NV_PERM_TWO_SAMPLE ? 3 : 2, NV_PERM_MAX_N);
  NV_CHECK_ARG(c && max_stat && max_t && count_unc && count_fwe && p_unc && p_fwe && workspace, "nv_perm_finish: null pointer");
  NV_CHECK_ARG(R >= 1 && R <= NV_PERM_MAX_R && V >= 1, "nv_perm_finish: R=%d outside [1, %d] or V=%d not positive", R, NV_PERM_MAX_R, V);
  NV_CHECK_ARG(splits >= 0 && splits <= NV_PERM_MAX_SPLITS, "nv_perm_finish: splits=%d outside [0, %d] (0 = automatic)", splits, NV_PERM_MAX_SPLITS);
  NV_CHECK_ARG(n_alphas >= 0 && n_alphas <= NV_PERM_MAX_ALPHAS && (n_alphas == 0 || (alphas && critical_t)), "nv_perm_finish: n_alphas=%d outside [0, %d], or alphas / critical_t missing",
               n_alphas, NV_PERM_MAX_ALPHAS);
  NV_CHECK_ARG(nv_aligned(c, 4) && nv_aligned(max_stat, 4) && nv_aligned(max_t, 4) && nv_aligned(count_unc, 4) && nv_aligned(count_fwe, 4) && nv_aligned(p_unc, 4) &&
                   nv_aligned(p_fwe, 4) && nv_aligned(critical_t, 4) && nv_aligned16(workspace),
               "nv_perm_finish: every array 4-byte aligned, the workspace 16-byte aligned");
  PermRanks ranks;
  ranks.n = n_alphas;
  for (int j = 0; j < NV_PERM_MAX_ALPHAS; ++j) ranks.k[j] = 1;
  for (int j = 0; j < n_alphas; ++j) {
    NV_CHECK_ARG(alphas[j] > 0.0 && alphas[j] < 1.0, "nv_perm_finish: alpha[%d] = %g outside (0, 1)", j, alphas[j]);
    ranks.k[j] = nv_perm_rank(alphas[j], R);
  }
  const int S = perm_resolve_splits(R, V, splits);
  const PermWs w = perm_ws(R, V, S);
  NV_CHECK_ARG(ws_bytes >= w.words * 4L, "nv_perm_finish: %d splits need a workspace of %ld bytes (nv_perm_workspace_bytes), got %ld", S, w.words * 4L, ws_bytes);
  const double df = (double)(kind == NV_PERM_TWO_SAMPLE ? N - 2 : N - 1);
  const int nvt = perm_vtiles(V), nvb = (V + FIN_THREADS - 1) / FIN_THREADS;
  float* ws = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(perm_rowmax_kernel, dim3((R + 3) / 4), dim3(256), 0, s, ws + w.pmax, R, nvt, df, max_stat, max_t);
  hipLaunchKernelGGL(perm_pvalue_kernel, dim3(nvb + 1), dim3(FIN_THREADS), 0, s, max_stat, R, V, S, c, ws + w.stat0, (const unsigned*)(ws + w.cnt), df, ranks, count_unc,
                     count_fwe, p_unc, p_fwe, critical_t);
  NV_CHECK_LAUNCH("nv_perm_finish");
  return NV_OK;
}
