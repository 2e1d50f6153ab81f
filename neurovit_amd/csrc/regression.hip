// The regression objective outside the fused head step: the standalone loss (nv_reg_loss) and the validation metrics on the raw scale
// (nv_reg_metrics_*).  The definition is in the header; the row body (reg_row_term, common.h) is the one of the head step's regression
// form (norm.hip), so both give the same bits.
#include "common.h"

// One workgroup forms the denominator D, then walks the rows with reg_row_term - the body and the order of the head step's two launches:
// each row's term is divided by D on its own, the terms are added in row order.
__global__ __launch_bounds__(256) void reg_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target, int B, int K, float grad_scale,
                                                       const float* __restrict__ scale_state, const RegLoss o, float* __restrict__ loss,
                                                       float* __restrict__ dpred) {
  __shared__ float red[4];
  __shared__ double redd[4];
  if (scale_state) grad_scale *= scale_state[LS_SCALE];      // dynamic loss scale: the gradients carry it, the reported loss does not
  const float D = (float)reg_denominator(target, o, B, K, redd);
  const float gs = D == 0.f ? 0.f : grad_scale / D;
  float total = 0.f;
  for (int b = 0; b < B; ++b) {
    const float num = reg_row_term(pred + (long)b * K, target, o, b, B, K, gs, red, dpred ? dpred + (long)b * K : nullptr);
    total += D == 0.f ? 0.f : num / D;
  }
  if (threadIdx.x == 0) loss[0] = total;
}

extern "C" int nv_reg_loss(const float* pred, const float* target, int B, int K, float grad_scale, const float* scale_state, const nv_reg_opts* opts,
                           float* loss, float* dpred, void* stream) {
  NV_CHECK_ARG(B > 0 && K > 0 && pred && target && loss, "nv_reg_loss: bad args (null pointer, or B / K not positive)");
  if (int rc = check_reg_opts(opts, "nv_reg_loss")) return rc;
  hipLaunchKernelGGL(reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, target, B, K, grad_scale, scale_state, make_reg_loss(opts), loss, dpred);
  NV_CHECK_LAUNCH("nv_reg_loss");
  return NV_OK;
}

// ---- metrics: workgroup k = target k.  Thread t sums the rows t, t + 256, ... in double, then the wave butterflies, then the four waves in
// order; thread 0 adds the nine sums to state[k].  One fixed order, no atomics.
__global__ __launch_bounds__(256) void reg_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target, int B, int K,
                                                          const float* __restrict__ mean, const float* __restrict__ std, double* __restrict__ state) {
  __shared__ double redd[NV_REG_METRIC_SLOTS][4];
  const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float m = mean ? mean[k] : 0.f, s = std ? std[k] : 1.f;
  double acc[NV_REG_METRIC_SLOTS];
#pragma unroll
  for (int i = 0; i < NV_REG_METRIC_SLOTS; ++i) acc[i] = 0.0;
  for (int b = tid; b < B; b += 256) {
    const float y = target[(long)b * K + k];
    if (!__builtin_isfinite(y)) continue;
    const float yh = __fadd_rn(__fmul_rn(pred[(long)b * K + k], s), m);
    const double e = (double)yh - (double)y, a = (double)y - (double)m, p = (double)yh - (double)m;
    acc[0] += 1.0; acc[1] += e; acc[2] += fabs(e); acc[3] += e * e;
    acc[4] += a; acc[5] += p; acc[6] += a * a; acc[7] += p * p; acc[8] += a * p;
  }
#pragma unroll
  for (int i = 0; i < NV_REG_METRIC_SLOTS; ++i) {
    const double v = wave_sum(acc[i]);
    if (lane == 0) redd[i][wid] = v;
  }
  __syncthreads();
  if (tid < NV_REG_METRIC_SLOTS) state[(long)k * NV_REG_METRIC_SLOTS + tid] += (redd[tid][0] + redd[tid][1]) + (redd[tid][2] + redd[tid][3]);
}

__global__ void reg_metrics_finish_kernel(const double* __restrict__ state, int K, float* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double* s = state + (long)k * NV_REG_METRIC_SLOTS;
  const double n = s[0], nan = (double)__builtin_nanf("");
  const double vy = s[6] - s[4] * s[4] / n, vp = s[7] - s[5] * s[5] / n, cov = s[8] - s[4] * s[5] / n;      // sums of squares about the means
  float* o = out + (long)k * 6;
  o[0] = (float)n;
  o[1] = (float)(n > 0.0 ? s[2] / n : nan);
  o[2] = (float)(n > 0.0 ? sqrt(s[3] / n) : nan);
  o[3] = (float)(n > 0.0 ? s[1] / n : nan);
  const bool y_var = n >= 2.0 && vy > 1e-12 * s[6], p_var = n >= 2.0 && vp > 1e-12 * s[7];      // (below that: the rounding of the double sums, no variance)
  o[4] = (float)((y_var && p_var) ? cov / sqrt(vy * vp) : nan);
  o[5] = (float)(y_var ? 1.0 - s[3] / vy : nan);
}

extern "C" int nv_reg_metrics_update(const float* pred, const float* target, int B, int K, const float* mean, const float* std, double* state, void* stream) {
  NV_CHECK_ARG(B > 0 && K > 0 && pred && target && state && nv_aligned(state, 8), "nv_reg_metrics_update: bad args (null pointer, B / K not positive, or state not 8-byte aligned)");
  hipLaunchKernelGGL(reg_metrics_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, pred, target, B, K, mean, std, state);
  NV_CHECK_LAUNCH("nv_reg_metrics_update");
  return NV_OK;
}

extern "C" int nv_reg_metrics_finish(const double* state, int K, float* out, void* stream) {
  NV_CHECK_ARG(K > 0 && state && out, "nv_reg_metrics_finish: bad args");
  hipLaunchKernelGGL(reg_metrics_finish_kernel, dim3((K + 255) / 256), dim3(256), 0, (hipStream_t)stream, state, K, out);
  NV_CHECK_LAUNCH("nv_reg_metrics_finish");
  return NV_OK;
}
