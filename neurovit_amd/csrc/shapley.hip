// Shapley value sampling on the device (Castro et al.; NeuroEncoder.shapley_values): the steps around the forward.  The players are
// patch tokens, blocks of them or atlas regions on the patch grid; the forward is the engine's and the masked copies are
// nv_mask_patches_rows' (perturb.hip).  This file draws the permutations, turns them into label rows, and accumulates the marginal
// contributions of the scored copies.
//
//   nv_shapley_ranks      (seed, unit, sample) -> ranks int32 [U R, B, F]: one workgroup per (unit, sample), keys ranked in LDS as
//                         nv_mim_labels ranks its units; row 1 of a unit (R = 2) is the antithetic permutation F - 1 - rank
//   nv_shapley_labels     ranks [Rows, F] + features [B, N] -> labels [Rows, N]: the rank of every patch's player (F for a patch of no player)
//   nv_shapley_accumulate scores of every prefix of every permutation -> values, standard errors, the efficiency residual; one thread
//                         owns (volume, player) and sums in double in unit order
//   nv_shapley_token_maps values [B, F] + features [B, N] -> maps [B, N]: a player's value spread evenly over its patches
//
// No atomics: every output cell is owned by one thread, and two runs give the same bits.  Contraction is off in the whole file: every
// double operation below is rounded on its own.
#include "attr_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int SR_THREADS = 256;
constexpr int SH_MAX_PLAYERS = 4096;     // 16 KB of keys in LDS
constexpr uint64_t SHAPLEY_DOMAIN = 0x53484150ull;         // ABI: the header states the draw rule
constexpr uint64_t SHAPLEY_STRIDE = 4096;

// Grid (B, U).  The key of player f is the top 24 bits of its draw as an fp32 in [0, 1) (exact); the players are ranked by
// nv_token_ranks' rule (descending, ties to the lower index) with its counting pass over the keys in LDS (every lane of a wave reads the
// same four keys per 16-byte read; the slots behind F hold key 0, which no key of a value >= 0 has and no comparison counts).
__global__ __launch_bounds__(SR_THREADS) void shapley_ranks_kernel(uint64_t seed, uint64_t first_unit, int R, int B, int F, int* __restrict__ ranks) {
  __shared__ u32x4 keys4[SH_MAX_PLAYERS / 4];
  unsigned* keys = reinterpret_cast<unsigned*>(keys4);
  const int tid = threadIdx.x, b = blockIdx.x, u = blockIdx.y;
  const int F4 = (F + 3) >> 2;
  const uint64_t seed_s = nv_hash64(seed, SHAPLEY_DOMAIN);
  const uint64_t counter = (((first_unit + (uint64_t)u) << 32) + (uint64_t)b) * SHAPLEY_STRIDE;
  for (int f = tid; f < 4 * F4; f += SR_THREADS) {
    const float key = (float)(unsigned)(nv_hash64(seed_s, counter + (uint64_t)f) >> 40) * 0x1p-24f;
    keys[f] = f < F ? float_key(key) : 0u;
  }
  __syncthreads();
  int* row0 = ranks + ((long)u * R * B + b) * F;
  int* row1 = row0 + (long)B * F;
  for (int f = tid; f < F; f += SR_THREADS) {
    const unsigned mine = keys[f];
    int above = 0;
    for (int j4 = 0; j4 < F4; ++j4) {
      const u32x4 k = keys4[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) above += (k[e] > mine || (k[e] == mine && 4 * j4 + e < f)) ? 1 : 0;
    }
    row0[f] = above;
    if (R == 2) row1[f] = F - 1 - above;
  }
}

// One thread per cell of labels [Rows, N]: row q belongs to volume q mod B.
__global__ void shapley_labels_kernel(const int* __restrict__ ranks, const int* __restrict__ features, long total, int B, int F, int N,
                                      int* __restrict__ labels) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long q = i / N;
  const int t = (int)(i - q * N), b = (int)(q % B);
  const int f = features[(long)b * N + t];
  labels[i] = (f >= 0 && f < F) ? ranks[q * F + f] : F;
}

// One thread per (b, f), b-major.  s_k of permutation q: ends[b, 0] (k = 0), interior[q, b, k - 1] (0 < k < F), ends[b, 1] (k = F).
__global__ void shapley_accumulate_kernel(const float* __restrict__ interior, const float* __restrict__ ends, const int* __restrict__ ranks, int U, int R,
                                          int B, int F, float* __restrict__ values, float* __restrict__ err, double* __restrict__ sums) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * F) return;
  const int b = (int)(i / F), f = (int)(i - (long)b * F);
  const float s_empty = ends[2 * b], s_full = ends[2 * b + 1];
  double sum = 0.0, sumsq = 0.0;
  for (int u = 0; u < U; ++u) {
    double unit = 0.0;
    for (int r = 0; r < R; ++r) {
      const long q = (long)u * R + r;
      int rho = ranks[(q * B + b) * F + f];
      rho = min(max(rho, 0), F - 1);                         // (a permutation never needs it: no read outside the score row)
      const float* s = interior + (q * B + b) * (long)(F - 1);
      const float before = rho == 0 ? s_empty : s[rho - 1];
      const float after = rho == F - 1 ? s_full : s[rho];
      unit += (double)after - (double)before;
    }
    if (R == 2) unit = unit / 2.0;
    sum += unit;
    sumsq += unit * unit;
  }
  sums[2 * i] = sum;
  sums[2 * i + 1] = sumsq;
  const double n = (double)U;
  values[i] = (float)(sum / n);
  const double var = (sumsq - sum * sum / n) / (n - 1.0);
  err[i] = U == 1 ? __uint_as_float(0x7fc00000u) : (float)sqrt(fmax(var, 0.0) / n);      // one unit has no spread to estimate: NaN
}

// One thread per volume, after the sums: delta[b] = (sum_f sums[b, f, 0]) / U - (s_F - s_0), the sum in player order.
__global__ void shapley_delta_kernel(const double* __restrict__ sums, const float* __restrict__ ends, int U, int B, int F, float* __restrict__ delta) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double total = 0.0;
  for (int f = 0; f < F; ++f) total += sums[2 * ((long)b * F + f)];
  delta[b] = (float)(total / (double)U - ((double)ends[2 * b + 1] - (double)ends[2 * b]));
}

// One workgroup per volume: the patches of every player are counted in LDS by the thread that owns the player (a pass over the volume's
// features per player would be F N; instead every thread walks the N features once for the players f = tid, tid + 256, .. it owns ->
// ceil(F / 256) N reads of LDS per thread), then every patch divides.
constexpr int TM_THREADS = 256;
__global__ __launch_bounds__(TM_THREADS) void shapley_token_maps_kernel(const float* __restrict__ values, const int* __restrict__ features, int F, int N,
                                                                        float* __restrict__ maps) {
  __shared__ int feat[SH_MAX_PLAYERS];
  __shared__ int count[SH_MAX_PLAYERS];
  const int tid = threadIdx.x, b = blockIdx.x;
  for (int t = tid; t < N; t += TM_THREADS) feat[t] = features[(long)b * N + t];
  __syncthreads();
  for (int f = tid; f < F; f += TM_THREADS) {
    int c = 0;
    for (int t = 0; t < N; ++t) c += feat[t] == f ? 1 : 0;
    count[f] = c;
  }
  __syncthreads();
  for (int t = tid; t < N; t += TM_THREADS) {
    const int f = feat[t];
    maps[(long)b * N + t] = (f >= 0 && f < F) ? values[(long)b * F + f] / (float)count[f] : 0.f;
  }
}
}  // namespace

extern "C" int nv_shapley_ranks(unsigned long seed, unsigned long first_unit, int U, int R, int B, int F, int* ranks, void* stream) {
  NV_CHECK_ARG(ranks && U > 0 && B > 0, "nv_shapley_ranks: bad arguments (null ranks, or U / B not positive)");
  NV_CHECK_ARG(R == 1 || R == 2, "nv_shapley_ranks: R = %d is neither 1 nor 2 (the antithetic pair)", R);
  NV_CHECK_ARG(F >= 2 && F <= SH_MAX_PLAYERS, "nv_shapley_ranks: %d players outside [2, %d]", F, SH_MAX_PLAYERS);
  NV_CHECK_ARG(U <= 65535 && first_unit < (1UL << 32) && first_unit + (unsigned long)U <= (1UL << 32), "nv_shapley_ranks: at most 65535 units in one call, units below 2^32");
  NV_CHECK_ARG(nv_aligned(ranks, 4), "nv_shapley_ranks: ranks 4-byte aligned");
  hipLaunchKernelGGL(shapley_ranks_kernel, dim3(B, U), dim3(SR_THREADS), 0, (hipStream_t)stream, (uint64_t)seed, (uint64_t)first_unit, R, B, F, ranks);
  NV_CHECK_LAUNCH("nv_shapley_ranks");
  return NV_OK;
}

extern "C" int nv_shapley_labels(const int* ranks, const int* features, int Rows, int B, int F, int N, int* labels, void* stream) {
  NV_CHECK_ARG(ranks && features && labels && Rows > 0 && B > 0 && F > 0 && N > 0,
               "nv_shapley_labels: bad arguments (null pointer, or Rows / B / F / N not positive)");
  NV_CHECK_ARG(nv_aligned(ranks, 4) && nv_aligned(features, 4) && nv_aligned(labels, 4), "nv_shapley_labels: element-aligned buffers");
  const long total = (long)Rows * N;
  NV_CHECK_ARG((total + 255) / 256 < (1L << 31), "nv_shapley_labels: Rows N too large");
  hipLaunchKernelGGL(shapley_labels_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ranks, features, total, B, F, N, labels);
  NV_CHECK_LAUNCH("nv_shapley_labels");
  return NV_OK;
}

extern "C" int nv_shapley_accumulate(const float* interior, const float* ends, const int* ranks, int U, int R, int B, int F, float* values, float* std_err,
                                     float* delta, double* sums, void* stream) {
  NV_CHECK_ARG(interior && ends && ranks && values && std_err && delta && sums && U > 0 && B > 0,
               "nv_shapley_accumulate: bad arguments (null pointer, or U / B not positive)");
  NV_CHECK_ARG(R == 1 || R == 2, "nv_shapley_accumulate: R = %d is neither 1 nor 2", R);
  NV_CHECK_ARG(F >= 2 && F <= SH_MAX_PLAYERS, "nv_shapley_accumulate: %d players outside [2, %d]", F, SH_MAX_PLAYERS);
  NV_CHECK_ARG(nv_aligned(interior, 4) && nv_aligned(ends, 4) && nv_aligned(ranks, 4) && nv_aligned(values, 4) && nv_aligned(std_err, 4) &&
                   nv_aligned(delta, 4) && nv_aligned(sums, 8),
               "nv_shapley_accumulate: element-aligned buffers (sums 8-byte)");
  const long cells = (long)B * F;
  NV_CHECK_ARG((cells + 255) / 256 < (1L << 31), "nv_shapley_accumulate: B F too large");
  hipLaunchKernelGGL(shapley_accumulate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, interior, ends, ranks, U, R, B, F,
                     values, std_err, sums);
  hipLaunchKernelGGL(shapley_delta_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const double*)sums, ends, U, B, F, delta);
  NV_CHECK_LAUNCH("nv_shapley_accumulate");
  return NV_OK;
}

extern "C" int nv_shapley_token_maps(const float* values, const int* features, int B, int F, int N, float* maps, void* stream) {
  NV_CHECK_ARG(values && features && maps && B > 0 && F > 0 && N > 0, "nv_shapley_token_maps: bad arguments (null pointer, or B / F / N not positive)");
  NV_CHECK_ARG(F <= SH_MAX_PLAYERS && N <= SH_MAX_PLAYERS, "nv_shapley_token_maps: %d players / %d patches, the kernel takes at most %d of each", F, N,
               SH_MAX_PLAYERS);
  NV_CHECK_ARG(nv_aligned(values, 4) && nv_aligned(features, 4) && nv_aligned(maps, 4), "nv_shapley_token_maps: element-aligned buffers");
  hipLaunchKernelGGL(shapley_token_maps_kernel, dim3(B), dim3(TM_THREADS), 0, (hipStream_t)stream, values, features, F, N, maps);
  NV_CHECK_LAUNCH("nv_shapley_token_maps");
  return NV_OK;
}
