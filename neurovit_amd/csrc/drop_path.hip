// Stochastic depth (drop path; timm's DropPath): the per-sample factors of every residual branch of a ViT, drawn on the device.
//
//   nv_drop_path_draw  (seed, B, depth, rate, schedule) -> factors fp32 [depth][2][B]: entry (l, c, b) scales branch c (0 attention,
//                      1 FeedForward) of block l for sample b: x <- x + f[l, c, b] * Dropout(branch(LN(x))), f = 0 or 1 / (1 - q_l).
// The rule (restated in tests/drop_path_ref.py), a hash domain of its own - no dropout or augmentation draw is reused:
//   q_l    = rate * l / (depth - 1) in double (NV_DROP_PATH_LINEAR, timm's linspace(0, rate, depth); 0 when depth == 1), or rate (NV_DROP_PATH_CONSTANT)
//   seed_p = nv_hash64(seed, 0x50415448);   h = nv_hash64(seed_p, ((2 l + c) << 32) + b)
//   kept iff (h >> 48) >= (unsigned)(q_l * 65536.0);   f = 1.0f / (1.0f - (float)q_l) when kept, else 0;   threshold 0: 1.0f, nothing hashed
// The kernels that apply the table are the path-aware forms of the four residual sites (common.h::PathCfg); nothing is read back.
#include "common.h"

#pragma clang fp contract(off)

namespace {
constexpr int DP_THREADS = 256;
constexpr uint64_t DP_DOMAIN = 0x50415448ull;      // "PATH"

// blockIdx.y = site 2 l + c, threads across the samples
__global__ __launch_bounds__(DP_THREADS) void drop_path_draw_kernel(uint64_t seed, int B, int depth, double rate, int schedule, float* __restrict__ factors) {
  const int b = blockIdx.x * DP_THREADS + threadIdx.x;
  if (b >= B) return;
  const int site = blockIdx.y, l = site >> 1;
  double q = rate;
  if (schedule == NV_DROP_PATH_LINEAR) q = depth > 1 ? rate * (double)l / (double)(depth - 1) : 0.0;
  const unsigned thresh = (unsigned)(q * 65536.0);
  float f = 1.0f;
  if (thresh) {
    const uint64_t h = nv_hash64(nv_hash64(seed, DP_DOMAIN), ((uint64_t)site << 32) + (uint64_t)b);
    f = ((unsigned)(h >> 48) >= thresh) ? 1.0f / (1.0f - (float)q) : 0.f;
  }
  factors[(long)site * B + b] = f;
}
}  // namespace

extern "C" int nv_drop_path_draw(unsigned long seed, int B, int depth, float rate, int schedule, float* factors, void* stream) {
  NV_CHECK_ARG(B > 0 && depth > 0 && 2L * depth <= 65535, "nv_drop_path_draw: B = %d, depth = %d (both positive, depth <= 32767)", B, depth);
  NV_CHECK_ARG(rate >= 0.f && rate < 1.f, "nv_drop_path_draw: rate %g outside [0, 1)", (double)rate);
  NV_CHECK_ARG(schedule == NV_DROP_PATH_LINEAR || schedule == NV_DROP_PATH_CONSTANT, "nv_drop_path_draw: schedule %d (NV_DROP_PATH_LINEAR = 0, NV_DROP_PATH_CONSTANT = 1)", schedule);
  NV_CHECK_ARG(factors && nv_aligned(factors, 4), "nv_drop_path_draw: factors is NULL or not 4-byte aligned");
  hipLaunchKernelGGL(drop_path_draw_kernel, dim3((B + DP_THREADS - 1) / DP_THREADS, 2 * depth), dim3(DP_THREADS), 0, (hipStream_t)stream, (uint64_t)seed, B, depth, (double)rate,
                     schedule, factors);
  NV_CHECK_LAUNCH("nv_drop_path_draw");
  return NV_OK;
}
