// Frozen-feature evaluation of the encoder: pooled features (nv_pool_features), a fused similarity + top-k search over a feature bank
// (nv_knn_topk) and the weighted k-nearest-neighbour vote (nv_knn_vote); the per-segment means are in segments.hip.  The definitions are in
// the header.  Nothing here reads back, nothing uses atomics; every sum has one fixed order, so the bits reproduce from run to run.
#include <math.h>

#include "eval_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ pooling
// One workgroup per sample.  The pooled row goes through LDS (d floats) so that the normalisation can walk it in column order.
//   mode 0: the cls row, copied.   mode 1: nv_token_mean's order - four partial sums over the rows t = g, g + 4, ... in fp32,
//   ((p0 + p1) + (p2 + p3)) / n.   mode 2: rows 1 .. n - 1 summed in double in ascending order, divided by n - 1 in double, rounded once.
__global__ __launch_bounds__(256) void pool_features_kernel(const float* __restrict__ tok, long batch_stride, long row_stride, int n, int d, int mode,
                                                            int normalize, float* __restrict__ out, long ldo, long row0) {
  extern __shared__ __attribute__((aligned(16))) float prow[];      // [d]
  __shared__ double inv_norm;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = tok + (long)b * batch_stride;
  for (int c = tid; c < d; c += 256) {
    float v;
    if (mode == 0) {
      v = x[c];
    } else if (mode == 1) {
      float p[4] = {0.f, 0.f, 0.f, 0.f};
      for (int g = 0; g < 4; ++g)
        for (int t = g; t < n; t += 4) p[g] = __fadd_rn(p[g], x[(long)t * row_stride + c]);
      v = __fdiv_rn(__fadd_rn(__fadd_rn(p[0], p[1]), __fadd_rn(p[2], p[3])), (float)n);
    } else {
      double s = 0.0;
      for (int t = 1; t < n; ++t) s += (double)x[(long)t * row_stride + c];
      v = (float)(s / (double)(n - 1));
    }
    prow[c] = v;
  }
  __syncthreads();
  float* o = out + (row0 + b) * ldo;
  if (!normalize) {
    for (int c = tid; c < d; c += 256) o[c] = prow[c];
    return;
  }
  if (tid == 0) {      // F.normalize: one chain in column order (d dependent double adds: microseconds, once per sample)
    double ss = 0.0;
    for (int c = 0; c < d; ++c) ss = __fma_rn((double)prow[c], (double)prow[c], ss);
    inv_norm = fmax(sqrt(ss), 1e-12);
  }
  __syncthreads();
  const double nrm = inv_norm;
  for (int c = tid; c < d; c += 256) o[c] = (float)((double)prow[c] / nrm);
}

// ------------------------------------------------------------------------------------------------ top-k
// A best-k list lives across the 64 lanes of one wave: lane l holds the entries at positions l and l + 64 (k <= 128), best first.  An empty
// slot is (sim -inf, idx -1).  Candidates of one list arrive in ascending bank index, so on equal sim the entry already in the list wins:
// the candidate's place is the number of entries with sim >= its own.  Returns whether the candidate entered.
struct KnnList {
  float s0, s1;
  int i0, i1;
};

__device__ __forceinline__ bool knn_insert(KnnList& L, float cv, int ci, int k, int lane) {
  // the candidate must beat the entry at k - 1 (strictly: that entry has the lower index), or find that slot empty
  const float ls = (k - 1 < 64) ? __shfl(L.s0, k - 1, 64) : __shfl(L.s1, k - 65, 64);
  const int li = (k - 1 < 64) ? __shfl(L.i0, k - 1, 64) : __shfl(L.i1, k - 65, 64);
  if (!(li < 0 || cv > ls)) return false;
  const int pos = __popcll(__ballot(L.i0 >= 0 && L.s0 >= cv)) + __popcll(__ballot(L.i1 >= 0 && L.s1 >= cv));
  const float p0s = __shfl_up(L.s0, 1, 64), up1s = __shfl_up(L.s1, 1, 64), w0s = __shfl(L.s0, 63, 64);
  const int p0i = __shfl_up(L.i0, 1, 64), up1i = __shfl_up(L.i1, 1, 64), w0i = __shfl(L.i0, 63, 64);
  const float p1s = lane == 0 ? w0s : up1s;
  const int p1i = lane == 0 ? w0i : up1i;
  if (lane == pos) { L.s0 = cv; L.i0 = ci; }
  else if (lane > pos) { L.s0 = p0s; L.i0 = p0i; }
  if (lane + 64 == pos) { L.s1 = cv; L.i1 = ci; }
  else if (lane + 64 > pos) { L.s1 = p1s; L.i1 = p1i; }
  if (lane >= k) { L.s0 = -INFINITY; L.i0 = -1; }
  if (lane + 64 >= k) { L.s1 = -INFINITY; L.i1 = -1; }
  return true;
}

// Workgroup = 4 waves, a 64-query x 64-bank-row similarity tile per step, 2 x 2 waves of 32 x 32 (four 16 x 16 MFMA blocks each), operands
// staged through LDS in 32-deep slices exactly as in gemm_f32_nt_kernel (precise.hip): whole 128-byte lines, two buffers, one barrier per
// slice.  blockIdx.y = the split: a contiguous range of bank tiles.  After the last slice of a tile the accumulators go to LDS (over the
// staging buffers), and wave w selects for the query rows 16 w .. 16 w + 15: lane c holds bank row n0 + c, one ballot against the row's
// k-th entry finds the few candidates that can enter, and each is placed with knn_insert.  The order in which a dot product is accumulated
// is the slice / MFMA order over d alone: it does not depend on the tile, the split or the row's place in either.
constexpr int KT = 64, KBK = 32, KLD = KBK + 4, KBUF = 2 * KT * KLD, KSL = KT + 1;

__global__ __launch_bounds__(256) void knn_topk_kernel(const float* __restrict__ Q, long ldq, int Nq, const float* __restrict__ bank, long ldb, int Nb,
                                                       int d, int k, const int* __restrict__ q_group, const int* __restrict__ b_group,
                                                       int tiles_per_split, int ntiles, int* __restrict__ oidx, float* __restrict__ osim) {
  extern __shared__ __attribute__((aligned(16))) float ksm[];      // [2][128][KLD] staging (the 64 x 65 sim tile lies over it) | [64][k] sims | [64][k] indices
  float* stile = ksm;
  float* lsim = ksm + 2 * KBUF;
  int* lidx = reinterpret_cast<int*>(lsim + KT * k);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m0 = blockIdx.x * KT;
  const int t_begin = blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);
  for (int e = tid; e < KT * k; e += 256) { lsim[e] = -INFINITY; lidx[e] = -1; }
  const int srow = tid >> 3, sch = tid & 7;
  const float* ap[2];
  const float* bp[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) ap[u] = Q + (long)min(m0 + srow + 32 * u, Nq - 1) * ldq + 4 * sch;
  f32x4 ra[2], rb[2];
  auto ld4 = [&](const float* p, int k0) -> f32x4 { return (k0 + 4 * sch < d) ? *reinterpret_cast<const f32x4*>(p + k0) : f32x4{0.f, 0.f, 0.f, 0.f}; };
  auto gload = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) { ra[u] = ld4(ap[u], k0); rb[u] = ld4(bp[u], k0); }
  };
  auto swrite = [&](float* buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<f32x4*>(buf + (srow + 32 * u) * KLD + 4 * sch) = ra[u];
      *reinterpret_cast<f32x4*>(buf + (KT + srow + 32 * u) * KLD + 4 * sch) = rb[u];
    }
  };
  const int wm = wid >> 1, wn = wid & 1, i = lane & 15, g = lane >> 4;
  const int nk = (d + KBK - 1) / KBK;
  __syncthreads();      // the lists are initialised
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int n0 = tile * KT;
#pragma unroll
    for (int u = 0; u < 2; ++u) bp[u] = bank + (long)min(n0 + srow + 32 * u, Nb - 1) * ldb + 4 * sch;
    f32x4 acc[2][2];
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn) acc[bm][bn] = f32x4{0.f, 0.f, 0.f, 0.f};
    gload(0);
    swrite(ksm);
    __syncthreads();
    for (int s = 0; s < nk; ++s) {
      const float* cur = ksm + (s & 1) * KBUF;
      if (s + 1 < nk) gload((s + 1) * KBK);
      const float* a0 = cur + (wm * 32 + i) * KLD + 4 * g;
      const float* b0 = cur + (KT + wn * 32 + i) * KLD + 4 * g;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        f32x4 af[2], bf[2];
#pragma unroll
        for (int bm = 0; bm < 2; ++bm) af[bm] = *reinterpret_cast<const f32x4*>(a0 + 16 * bm * KLD + 16 * ks);
#pragma unroll
        for (int bn = 0; bn < 2; ++bn) bf[bn] = *reinterpret_cast<const f32x4*>(b0 + 16 * bn * KLD + 16 * ks);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int bm = 0; bm < 2; ++bm)
#pragma unroll
            for (int bn = 0; bn < 2; ++bn) acc[bm][bn] = mfma4(bf[bn][t], af[bm][t], acc[bm][bn]);
      }
      if (s + 1 < nk) swrite(ksm + ((s + 1) & 1) * KBUF);
      __syncthreads();
    }
    // lane (j = i, q = g), register r of block (bm, bn) holds sim[query 16 (2 wm + bm) + j][bank row 16 (2 wn + bn) + 4 q + r]; every wave has
    // passed the last slice's barrier, so the staging buffers are free
#pragma unroll
    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
      for (int bn = 0; bn < 2; ++bn)
#pragma unroll
        for (int r = 0; r < 4; ++r) stile[(16 * (2 * wm + bm) + i) * KSL + 16 * (2 * wn + bn) + 4 * g + r] = acc[bm][bn][r];
    __syncthreads();
    const int j = n0 + lane;
    const int bg = (b_group && j < Nb) ? b_group[j] : -1;
    for (int r = 0; r < 16; ++r) {
      const int row = 16 * wid + r, q = m0 + row;
      if (q >= Nq) break;
      const float v = stile[row * KSL + lane];
      const int qg = (q_group && b_group) ? q_group[q] : -1;
      const bool ok = j < Nb && !(qg >= 0 && qg == bg);
      const float last_s = lsim[row * k + k - 1];
      const int last_i = lidx[row * k + k - 1];
      unsigned long long mask = __ballot(ok && (last_i < 0 || v > last_s));
      if (mask == 0ull) continue;
      KnnList L;
      L.s0 = lane < k ? lsim[row * k + lane] : -INFINITY;
      L.i0 = lane < k ? lidx[row * k + lane] : -1;
      L.s1 = lane + 64 < k ? lsim[row * k + lane + 64] : -INFINITY;
      L.i1 = lane + 64 < k ? lidx[row * k + lane + 64] : -1;
      while (mask) {
        const int c = __builtin_ctzll(mask);
        mask &= mask - 1;
        knn_insert(L, __shfl(v, c, 64), n0 + c, k, lane);
      }
      if (lane < k) { lsim[row * k + lane] = L.s0; lidx[row * k + lane] = L.i0; }
      if (lane + 64 < k) { lsim[row * k + lane + 64] = L.s1; lidx[row * k + lane + 64] = L.i1; }
    }
    __syncthreads();      // the sim tile is consumed before the next tile's first slice lands on it
  }
  // each wave wrote the lists of its own 16 rows (or the initial fill, behind the first barrier)
  const long obase = ((long)blockIdx.y * Nq) * k;
  for (int r = 0; r < 16; ++r) {
    const int row = 16 * wid + r, q = m0 + row;
    if (q >= Nq) break;
    for (int p = lane; p < k; p += 64) {
      osim[obase + (long)q * k + p] = lsim[row * k + p];
      oidx[obase + (long)q * k + p] = lidx[row * k + p];
    }
  }
}

// One wave per query row: the lists of the splits, in split order (= ascending bank index), through the same knn_insert.
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ wsim, const int* __restrict__ widx, int Nq, int k, int splits,
                                                        int* __restrict__ idx, float* __restrict__ sim) {
  const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= Nq) return;
  KnnList L{-INFINITY, -INFINITY, -1, -1};
  for (int s = 0; s < splits; ++s) {
    const long base = ((long)s * Nq + q) * k;
    const float c0s = lane < k ? wsim[base + lane] : -INFINITY, c1s = lane + 64 < k ? wsim[base + lane + 64] : -INFINITY;
    const int c0i = lane < k ? widx[base + lane] : -1, c1i = lane + 64 < k ? widx[base + lane + 64] : -1;
    for (int p = 0; p < k; ++p) {
      const float cv = p < 64 ? __shfl(c0s, p, 64) : __shfl(c1s, p - 64, 64);
      const int ci = p < 64 ? __shfl(c0i, p, 64) : __shfl(c1i, p - 64, 64);
      if (ci < 0) break;      // the rest of this split's list is empty
      if (!knn_insert(L, cv, ci, k, lane)) break;      // ... or loses too: a split's list is sorted, what follows is no better and has a higher index or a lower sim
    }
  }
  if (lane < k) { sim[(long)q * k + lane] = L.s0; idx[(long)q * k + lane] = L.i0; }
  if (lane + 64 < k) { sim[(long)q * k + lane + 64] = L.s1; idx[(long)q * k + lane + 64] = L.i1; }
}

constexpr int KNN_MAX_K = 128, KNN_MAX_SPLITS = 64;
// (not nv_resolve_splits, on purpose: an explicit request is returned as given, and a split holds at least two bank tiles)
int knn_resolve_splits(int Nq, int Nb, int splits) {
  if (splits > 0) return splits;
  const int qtiles = (Nq + KT - 1) / KT, ntiles = (Nb + KT - 1) / KT;
  int s = (1024 + qtiles - 1) / qtiles;      // about four workgroups per CU
  if (s > ntiles / 2) s = ntiles / 2;         // at least two bank tiles per split: below that the merge costs more than the split gains
  if (s > KNN_MAX_SPLITS) s = KNN_MAX_SPLITS;
  return s < 1 ? 1 : s;
}

// ------------------------------------------------------------------------------------------------ vote
// One wave per query.  w[i] (fp32) for the first k slots into LDS; a slot is usable when 0 <= idx < Nb (and, classification, its label lies in
// [0, C); regression, per column, its target is not NaN).
__device__ __forceinline__ float knn_weight(int weighting, float s, float s0, float T) { return weighting ? expf((s - s0) / T) : 1.f; }

__global__ __launch_bounds__(64) void knn_vote_cls_kernel(const int* __restrict__ idx, const float* __restrict__ sim, int kmax, int k, int weighting, float T,
                                                          int Nb, const int* __restrict__ labels, int C, float* __restrict__ scores, int* __restrict__ pred) {
  __shared__ float w[KNN_MAX_K];
  __shared__ int lab[KNN_MAX_K];
  const int q = blockIdx.x, lane = threadIdx.x;
  const float s0 = sim[(long)q * kmax];
  for (int i = lane; i < k; i += 64) {
    const int j = idx[(long)q * kmax + i];
    int l = -1;
    if (j >= 0 && j < Nb) { l = labels[j]; if (!valid_label(l, C)) l = -1; }
    lab[i] = l;
    w[i] = l >= 0 ? knn_weight(weighting, sim[(long)q * kmax + i], s0, T) : 0.f;
  }
  __syncthreads();
  double total = 0.0;
  for (int i = 0; i < k; ++i)
    if (lab[i] >= 0) total += (double)w[i];
  double best = -1.0;
  int best_c = -1;
  for (int c = lane; c < C; c += 64) {
    double s = 0.0;
    for (int i = 0; i < k; ++i)
      if (lab[i] == c) s += (double)w[i];
    const double sc = total > 0.0 ? s / total : 0.0;
    scores[(long)q * C + c] = (float)sc;
    if (total > 0.0 && sc > best) { best = sc; best_c = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {      // arg-max under (score larger, class lower): a total order, so the butterfly's pairing does not matter
    const double ob = __shfl_xor(best, o, 64);
    const int oc = __shfl_xor(best_c, o, 64);
    if (oc >= 0 && (best_c < 0 || ob > best || (ob == best && oc < best_c))) { best = ob; best_c = oc; }
  }
  if (lane == 0) pred[q] = best_c;
}

__global__ __launch_bounds__(64) void knn_vote_reg_kernel(const int* __restrict__ idx, const float* __restrict__ sim, int kmax, int k, int weighting, float T,
                                                          int Nb, const float* __restrict__ targets, int K, float* __restrict__ pred) {
  __shared__ float w[KNN_MAX_K];
  __shared__ int nb[KNN_MAX_K];
  const int q = blockIdx.x, lane = threadIdx.x;
  const float s0 = sim[(long)q * kmax];
  for (int i = lane; i < k; i += 64) {
    const int j = idx[(long)q * kmax + i];
    const bool ok = j >= 0 && j < Nb;
    nb[i] = ok ? j : -1;
    w[i] = ok ? knn_weight(weighting, sim[(long)q * kmax + i], s0, T) : 0.f;
  }
  __syncthreads();
  for (int c = lane; c < K; c += 64) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < k; ++i) {
      if (nb[i] < 0) continue;
      const float t = targets[(long)nb[i] * K + c];
      if (t != t) continue;
      num += (double)w[i] * (double)t;
      den += (double)w[i];
    }
    pred[(long)q * K + c] = den > 0.0 ? (float)(num / den) : __builtin_nanf("");
  }
}

}  // namespace

extern "C" int nv_pool_features(const float* tokens, long batch_stride, long row_stride, int B, int n, int d, int mode, int normalize, float* out,
                                long ldo, long row0, void* stream) {
  NV_CHECK_ARG(tokens && out && B > 0 && n > 0 && d > 0 && d <= 8192, "nv_pool_features: null pointer or bad shape B=%d n=%d d=%d (d up to 8192)", B, n, d);
  NV_CHECK_ARG(mode == NV_POOL_CLS || mode == NV_POOL_MEAN || mode == NV_POOL_PATCH_MEAN, "nv_pool_features: unknown mode %d", mode);
  NV_CHECK_ARG(mode != NV_POOL_PATCH_MEAN || n >= 2, "nv_pool_features: the patch mean needs n >= 2 rows (a cls row and at least one patch), got n=%d", n);
  NV_CHECK_ARG(row_stride >= d && batch_stride >= 0 && ldo >= d && row0 >= 0, "nv_pool_features: row_stride=%ld and ldo=%ld must cover d=%d, row0=%ld >= 0", row_stride, ldo, d, row0);
  hipLaunchKernelGGL(pool_features_kernel, dim3(B), dim3(256), (size_t)d * sizeof(float), (hipStream_t)stream, tokens, batch_stride, row_stride, n, d, mode,
                     normalize ? 1 : 0, out, ldo, row0);
  NV_CHECK_LAUNCH("nv_pool_features");
  return NV_OK;
}

extern "C" int nv_knn_topk_splits(int Nq, int Nb, int splits) {
  if (Nq <= 0 || Nb <= 0 || splits < 0 || splits > KNN_MAX_SPLITS) return 0;
  return knn_resolve_splits(Nq, Nb, splits);
}

extern "C" long nv_knn_topk_workspace_bytes(int Nq, int Nb, int k, int splits) {
  const int s = nv_knn_topk_splits(Nq, Nb, splits);
  if (s <= 1 || k < 1 || k > KNN_MAX_K) return 0;
  return (long)s * Nq * k * (long)(sizeof(float) + sizeof(int));
}

extern "C" int nv_knn_topk(const float* Q, long ldq, int Nq, const float* bank, long ldb, int Nb, int d, int k, const int* q_group, const int* b_group,
                           int splits, int* idx, float* sim, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(Q && bank && idx && sim && Nq > 0 && Nb > 0 && d > 0, "nv_knn_topk: null pointer or bad shape Nq=%d Nb=%d d=%d", Nq, Nb, d);
  NV_CHECK_ARG(k >= 1 && k <= KNN_MAX_K, "nv_knn_topk: k=%d outside [1, %d]", k, KNN_MAX_K);
  NV_CHECK_ARG((d % 4) == 0 && (ldq % 4) == 0 && (ldb % 4) == 0 && ldq >= d && ldb >= d && nv_aligned16(Q) && nv_aligned16(bank),
               "nv_knn_topk: d=%d, ldq=%ld and ldb=%ld must be multiples of 4 with ld >= d, Q and bank 16-byte aligned", d, ldq, ldb);
  NV_CHECK_ARG(splits >= 0 && splits <= KNN_MAX_SPLITS, "nv_knn_topk: splits=%d outside [0, %d] (0 = automatic)", splits, KNN_MAX_SPLITS);
  NV_CHECK_ARG((q_group == nullptr) == (b_group == nullptr), "nv_knn_topk: q_group and b_group are given together or not at all");
  NV_CHECK_ARG(nv_aligned(q_group, 4) && nv_aligned(b_group, 4) && nv_aligned(idx, 4) && nv_aligned(sim, 4), "nv_knn_topk: idx, sim and the group arrays 4-byte aligned");
  NV_CHECK_ARG((long)Nq * k < (1L << 31), "nv_knn_topk: Nq * k = %ld does not fit the 32-bit offsets of the lists", (long)Nq * k);
  const int S = knn_resolve_splits(Nq, Nb, splits);
  const long need = nv_knn_topk_workspace_bytes(Nq, Nb, k, S);
  NV_CHECK_ARG(S == 1 || (workspace && ws_bytes >= need && nv_aligned(workspace, 4)), "nv_knn_topk: %d splits need a workspace of %ld bytes (nv_knn_topk_workspace_bytes), got %ld",
               S, need, workspace ? ws_bytes : 0L);
  const int qtiles = (Nq + KT - 1) / KT, ntiles = (Nb + KT - 1) / KT, tps = (ntiles + S - 1) / S;
  const size_t lds = (size_t)(2 * KBUF + 2 * KT * k) * sizeof(float);
  static_assert((size_t)(2 * KBUF + 2 * KT * KNN_MAX_K) * sizeof(float) <= 160 * 1024, "LDS budget");
  static_assert(KT * KSL <= 2 * KBUF, "the sim tile lies over the staging buffers");
  if (lds > 64 * 1024) {
    static bool allowed = false;
    if (int rc = allow_lds(knn_topk_kernel, (int)((2 * KBUF + 2 * KT * KNN_MAX_K) * sizeof(float)), allowed, "nv_knn_topk")) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  float* wsim = S == 1 ? sim : (float*)workspace;
  int* widx = S == 1 ? idx : (int*)((float*)workspace + (long)S * Nq * k);
  hipLaunchKernelGGL(knn_topk_kernel, dim3(qtiles, S), dim3(256), lds, s, Q, ldq, Nq, bank, ldb, Nb, d, k, q_group, b_group, tps, ntiles, widx, wsim);
  if (S > 1) hipLaunchKernelGGL(knn_merge_kernel, dim3((Nq + 3) / 4), dim3(256), 0, s, wsim, widx, Nq, k, S, idx, sim);
  NV_CHECK_LAUNCH("nv_knn_topk");
  return NV_OK;
}

extern "C" int nv_knn_vote(const int* idx, const float* sim, int Nq, int kmax, int k, int weighting, float temperature, int Nb, const int* labels, int C,
                           float* scores, int* pred, const float* targets, int K, float* pred_reg, void* stream) {
  NV_CHECK_ARG(idx && sim && Nq > 0 && Nb > 0, "nv_knn_vote: null pointer or bad shape Nq=%d Nb=%d", Nq, Nb);
  NV_CHECK_ARG(kmax >= 1 && kmax <= KNN_MAX_K && k >= 1 && k <= kmax, "nv_knn_vote: need 1 <= k=%d <= kmax=%d <= %d", k, kmax, KNN_MAX_K);
  NV_CHECK_ARG(weighting == NV_KNN_UNIFORM || weighting == NV_KNN_SOFTMAX, "nv_knn_vote: unknown weighting %d", weighting);
  NV_CHECK_ARG(weighting != NV_KNN_SOFTMAX || (temperature > 0.f && temperature < INFINITY), "nv_knn_vote: the softmax weights need a finite temperature > 0, got %g", (double)temperature);
  NV_CHECK_ARG((labels != nullptr) != (targets != nullptr), "nv_knn_vote: give labels (classification) or targets (regression), one of the two");
  hipStream_t s = (hipStream_t)stream;
  if (labels) {
    NV_CHECK_ARG(C >= 1 && scores && pred, "nv_knn_vote: classification needs C=%d >= 1, scores and pred", C);
    hipLaunchKernelGGL(knn_vote_cls_kernel, dim3(Nq), dim3(64), 0, s, idx, sim, kmax, k, weighting, temperature, Nb, labels, C, scores, pred);
  } else {
    NV_CHECK_ARG(K >= 1 && pred_reg, "nv_knn_vote: regression needs K=%d >= 1 and pred_reg", K);
    hipLaunchKernelGGL(knn_vote_reg_kernel, dim3(Nq), dim3(64), 0, s, idx, sim, kmax, k, weighting, temperature, Nb, targets, K, pred_reg);
  }
  NV_CHECK_LAUNCH("nv_knn_vote");
  return NV_OK;
}
