// Exponential moving average of a flat fp32 parameter arena (neurovit_amd.ModelEma), gfx950.  One HBM-bound streaming kernel.
//
//   nv_ema_update    ema[i] = ema[i] + (p[i] - ema[i]) * weight      (weight = float32(1 - decay), formed on the host)
//
// The difference, the product and the sum are each rounded on their own (no FMA), so the result is bit-equal to the same fp32 torch
// expression on the CPU (tests/ema_ref.py), and p == ema is an exact fixed point: frozen parameters and the constant slots of an
// arena never drift.  8 B/param read + 4 B/param written; no 16-bit shadow is written - the averaged model refreshes its own lazily.
#include "common.h"

#pragma clang fp contract(off)

#ifndef NV_EMA_UNROLL
#define NV_EMA_UNROLL 2            // float4 groups per thread per pass, all loads issued before the first use (NV_ADAMW_UNROLL's measured 2)
#endif

namespace {
// Streaming kernel as adamw_kernel (optim.hip): every byte is touched once per step, so both loads and the store carry the
// non-temporal hint; grid-stride, so that a capped grid (max_blocks) streams the range with a fraction of the chip's wave slots.
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ ema, const float* __restrict__ p, long n4, float weight) {
  constexpr int U = NV_EMA_UNROLL;
  for (long i0 = (long)blockIdx.x * blockDim.x * U + threadIdx.x; i0 < n4; i0 += (long)gridDim.x * blockDim.x * U) {
    f32x4 ev[U], pv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + (long)u * blockDim.x;
      if (i < n4) {
        ev[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(ema) + i);
        pv[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long i = i0 + (long)u * blockDim.x;
      if (i < n4) {
        const f32x4 d = pv[u] - ev[u];
        const f32x4 s = d * weight;
        __builtin_nontemporal_store(ev[u] + s, reinterpret_cast<f32x4*>(ema) + i);
      }
    }
  }
}
}  // namespace

// count must be a positive multiple of 4 (arena segments are padded); 0 <= weight <= 1.
extern "C" int nv_ema_update(float* ema, const float* p, long count, float weight, int max_blocks, void* stream) {
  NV_CHECK_ARG(ema && p && count > 0 && (count % 4) == 0, "nv_ema_update: null pointer, or count=%ld is not a positive multiple of 4", count);
  NV_CHECK_ARG(nv_aligned16(ema) && nv_aligned16(p), "nv_ema_update: ema and p must be 16-byte aligned");
  NV_CHECK_ARG(weight >= 0.f && weight <= 1.f, "nv_ema_update: weight=%g must be in [0, 1] (and not NaN)", (double)weight);
  const long n4 = count / 4;
  long blocks = (n4 + 256L * NV_EMA_UNROLL - 1) / (256L * NV_EMA_UNROLL);
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  hipLaunchKernelGGL(ema_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ema, p, n4, weight);
  NV_CHECK_LAUNCH("nv_ema_update");
  return NV_OK;
}
