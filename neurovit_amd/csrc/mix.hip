// The draws of Mixup / CutMix on the device (neurovit_amd.augment.VolumeMix), for 3D volumes and 4D series.  The pass that mixes a batch
// by these rows is nv_augment_mix (augment.hip), one body with the augmentation.
//
//   nv_mix_params    (config, seed, step, rank) -> mix int32 [B, NV_MIX_COLS]: {partner, mode, bits of the pixel lambda, bits of the label
//                    lambda, tries, x0, x1, y0, y1, z0, z1, 0}, drawn on the device with nv_hash64 in a domain of its own (the rule is in
//                    the header; tests/mix_ref.py restates it).  lambda ~ Beta(alpha, alpha) by Joehnk's rule in double; the CutMix box in fp32.
// The counter, the chance test and the box centre are the draw rule of augment.hip and affine.hip: augment_common.h.
#include "augment_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int MX_THREADS = 256;
constexpr int MX_TRIES = 64;

// ------------------------------------------------------------------------------------------------ parameters
struct MixDraw {
  int S[3];
  double inv_alpha_mixup, inv_alpha_cutmix;      // 0 = that mode is off
  unsigned prob_thresh, switch_thresh;           // (unsigned)(p * 65536)
};

__device__ __forceinline__ double unit_open(uint64_t h) { return ((double)(h >> 12) + 0.5) * 0x1p-52; }   // 52 bits + a half: exact, never 0

// One thread per sample: draw d of sample b at step s hashes the counter ((s 2^32 + b) 256 + d) mod 2^64 under the rank's mix seed.
__global__ __launch_bounds__(MX_THREADS) void mix_params_kernel(MixDraw cfg, uint64_t seed, uint64_t step, uint64_t rank, int B, int* __restrict__ mix) {
  const int b = blockIdx.x * MX_THREADS + threadIdx.x;
  if (b >= B) return;
  const SampleDraws h(seed, rank, MIX_DOMAIN, MIX_STRIDE, step, b);
  const int partner = B - 1 - b;
  int row[NV_MIX_COLS] = {partner, 0, __float_as_int(1.0f), __float_as_int(1.0f), 0, 0, 0, 0, 0, 0, 0, 0};
  int mode = 0;
  if (partner != b && draw_chance(h(0), cfg.prob_thresh)) {
    const bool mixup = cfg.inv_alpha_mixup != 0.0, cutmix = cfg.inv_alpha_cutmix != 0.0;
    if (mixup && cutmix) mode = draw_chance(h(1), cfg.switch_thresh) ? 2 : 1;
    else mode = cutmix ? 2 : (mixup ? 1 : 0);
  }
  if (mode) {
    const double inv_alpha = mode == 2 ? cfg.inv_alpha_cutmix : cfg.inv_alpha_mixup;
    double x = 0.0, y = 0.0;
    int t = 0;
    for (; t < MX_TRIES; ++t) {                                   // Joehnk: accept the first pair with x + y <= 1
      x = pow(unit_open(h(16 + 2 * t)), inv_alpha);
      y = pow(unit_open(h(17 + 2 * t)), inv_alpha);
      if (x + y <= 1.0) break;
    }
    const float lam = (float)(x / (x + y));
    row[1] = mode;
    row[2] = __float_as_int(lam);
    row[3] = row[2];
    row[4] = t < MX_TRIES ? t + 1 : MX_TRIES;
    if (mode == 2) {
      const float r = __fsqrt_rn(1.0f - lam);
      long cells = 1;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int S = cfg.S[a];
        const int e = (int)((float)S * r);
        const int c = draw_below(h(2 + a), S);
        const int lo = max(c - e / 2, 0), hi = min(c + e / 2, S);
        row[5 + 2 * a] = lo;
        row[6 + 2 * a] = hi;
        cells *= hi - lo;
      }
      const double total = (double)cfg.S[0] * (double)cfg.S[1] * (double)cfg.S[2];
      row[3] = __float_as_int((float)(1.0 - (double)cells / total));
    }
  }
#pragma unroll
  for (int i = 0; i < NV_MIX_COLS; ++i) mix[(long)NV_MIX_COLS * b + i] = row[i];
}

}  // namespace

extern "C" int nv_mix_params(const nv_mix_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* mix, void* stream) {
  NV_CHECK_ARG(cfg && mix && B > 0 && rank >= 0, "nv_mix_params: bad arguments (null pointer, B not positive or a negative rank)");
  NV_CHECK_ARG(cfg->struct_size == (int)sizeof(nv_mix_config), "nv_mix_params: struct_size %d, this library's nv_mix_config has %d bytes", cfg->struct_size,
               (int)sizeof(nv_mix_config));
  NV_CHECK_ARG(nv_aligned(mix, 4), "nv_mix_params: mix 4-byte aligned");
  MixDraw d;
  for (int a = 0; a < 3; ++a) {
    NV_CHECK_ARG(cfg->roi[a] > 0, "nv_mix_params: axis %d: roi %d must be positive", a, cfg->roi[a]);
    d.S[a] = cfg->roi[a];
  }
  const double alphas[2] = {cfg->mixup_alpha, cfg->cutmix_alpha};
  for (int m = 0; m < 2; ++m)
    NV_CHECK_ARG(alphas[m] == 0.0 || (alphas[m] >= 0.05 && alphas[m] <= 1.0), "nv_mix_params: %s alpha %g outside [0.05, 1] (0 = off)", m ? "cutmix" : "mixup", alphas[m]);
  NV_CHECK_ARG(cfg->prob >= 0.0 && cfg->prob <= 1.0 && cfg->switch_prob >= 0.0 && cfg->switch_prob <= 1.0, "nv_mix_params: prob %g / switch_prob %g outside [0, 1]",
               cfg->prob, cfg->switch_prob);
  d.inv_alpha_mixup = alphas[0] != 0.0 ? 1.0 / alphas[0] : 0.0;
  d.inv_alpha_cutmix = alphas[1] != 0.0 ? 1.0 / alphas[1] : 0.0;
  d.prob_thresh = chance_thresh(cfg->prob);
  d.switch_thresh = chance_thresh(cfg->switch_prob);
  hipLaunchKernelGGL(mix_params_kernel, dim3((B + MX_THREADS - 1) / MX_THREADS), dim3(MX_THREADS), 0, (hipStream_t)stream, d, (uint64_t)seed, (uint64_t)step,
                     (uint64_t)rank, B, mix);
  NV_CHECK_LAUNCH("nv_mix_params");
  return NV_OK;
}
