// Global-norm gradient clipping on the device (torch.nn.utils.clip_grad_norm_, norm_type 2), gfx950:
//   scaler.unscale_(opt); clip_grad_norm_(model.parameters(), c); scaler.step(opt)
// without a host read of the norm.  State: one caller-owned block of NV_GRAD_CLIP_BYTES (indices GC_*, common.h).  Per optimizer step:
//   nv_grad_sumsq         sumsq += sum of x^2 over one gradient buffer (fp32 or the 16-bit operand format), once per buffer; with a
//                         loss-scale state it also raises LS_FOUND_INF - the pass then stands in for nv_loss_scale_check
//   nv_loss_scale_update  (dynamic loss scale only) writes LS_UNSCALE of the gradients that were summed
//   nv_grad_clip_finish   total_norm = sqrt(sumsq) |grad_scale| unscale;  coef = min(max_norm / (total_norm + 1e-6), 1);  sumsq = 0
//   nv_adamw_step_clipped (optim.hip) multiplies its gradient factor by coef
// Every element is widened to double BEFORE it is squared and the sum is kept in double: finite fp32 gradients under a loss scale of
// 65536 have squares (1e30^2) and sums (1000 x 9e36) beyond fp32, and only in double is "the sum is not finite <=> an element is
// inf / NaN" exact (the largest finite sum, 2^31 x 3.4e38^2 = 2.5e86, is far inside the format).  The kernel is HBM-bound (354 MB for
// ViT3D-base); the conversions and FMAs in double are a few microseconds of VALU time beside it.
// Bits reproduce from run to run: no floating-point atomics - every workgroup stores ONE double partial (fixed order inside: four
// chains per lane, xor-shuffle tree, the four waves in index order) and a second, one-workgroup launch adds the partials in a fixed
// order onto the running sum.  The grid is a function of (count, max_blocks) alone, so the order is too.
#include "common.h"

constexpr int GC_UNROLL = 4;             // 16-byte loads in flight per lane
constexpr int GC_MAX_BLOCKS = NV_GRAD_CLIP_MAX_BLOCKS;

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
  const unsigned long long w = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __shfl_xor((unsigned)w, o, 64), hi = __shfl_xor((unsigned)(w >> 32), o, 64);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += shfl_xor_f64(v, o);
  return v;
}
__device__ __forceinline__ double sq_acc(double acc, float x) {
  const double d = (double)x;
  return __builtin_fma(d, d, acc);
}
// exponent bits all ones: inf or NaN (read as an integer - nothing for value-based reasoning to fold)
__device__ __forceinline__ bool nonfinite_f64(double v) {
  return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// E = float (G16 = false) or r16 holding T (G16 = true).  g is only element-aligned (stock parameter tensors are summed too): the first
// `head` elements up to the 16-byte boundary and the `count - head - VEC * nv` behind the last whole piece are read one by one by
// workgroup 0, everything between them in 16-byte non-temporal pieces, grid-stride.
template <bool G16, typename T>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const void* __restrict__ gp, long count, double* __restrict__ partials) {
  typedef typename std::conditional<G16, r16, float>::type E;
  constexpr int VEC = 16 / (int)sizeof(E);
  const E* g = reinterpret_cast<const E*>(gp);
  long head = (long)(((16u - (unsigned)((unsigned long)g & 15u)) & 15u) / sizeof(E));
  if (head > count) head = count;
  const long nv = (count - head) / VEC;
  const long tail0 = head + nv * VEC;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (long i0 = (long)blockIdx.x * 256 * GC_UNROLL + threadIdx.x; i0 < nv; i0 += (long)gridDim.x * 256 * GC_UNROLL) {
    if constexpr (G16) {
      const r16x8* gv = reinterpret_cast<const r16x8*>(g + head);
      r16x8 w[GC_UNROLL];
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) {
        const long i = i0 + u * 256;
        w[u] = r16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (i < nv) w[u] = __builtin_nontemporal_load(gv + i);
      }
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) {
        a0 = sq_acc(sq_acc(a0, dec1<T>(w[u][0])), dec1<T>(w[u][4]));
        a1 = sq_acc(sq_acc(a1, dec1<T>(w[u][1])), dec1<T>(w[u][5]));
        a2 = sq_acc(sq_acc(a2, dec1<T>(w[u][2])), dec1<T>(w[u][6]));
        a3 = sq_acc(sq_acc(a3, dec1<T>(w[u][3])), dec1<T>(w[u][7]));
      }
    } else {
      const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
      f32x4 w[GC_UNROLL];
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) {
        const long i = i0 + u * 256;
        w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < nv) w[u] = __builtin_nontemporal_load(gv + i);
      }
#pragma unroll
      for (int u = 0; u < GC_UNROLL; ++u) {
        a0 = sq_acc(a0, w[u][0]); a1 = sq_acc(a1, w[u][1]); a2 = sq_acc(a2, w[u][2]); a3 = sq_acc(a3, w[u][3]);
      }
    }
  }
  if (blockIdx.x == 0) {                 // head and tail: at most VEC - 1 elements each
    const long t = threadIdx.x;
    auto one = [&](long i) -> float {
      if constexpr (G16) return dec1<T>(g[i]);
      else return g[i];
    };
    if (t < head) a0 = sq_acc(a0, one(t));
    if (tail0 + t < count) a1 = sq_acc(a1, one(tail0 + t));
  }
  double s = wave_sum_f64((a0 + a1) + (a2 + a3));
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one workgroup: lane t adds partials t, t + 256, ... in rising order, then the same tree as above; the total goes ONTO the running
// sum (several buffers of one step accumulate through stream order).  ls (may be null): the loss-scale block - found_inf is raised when
// the running sum is not finite and left alone otherwise.
__global__ __launch_bounds__(256) void grad_sumsq_finish_kernel(float* __restrict__ st, int nparts, float* __restrict__ ls) {
  const double* partials = reinterpret_cast<const double*>(st + GC_PARTIALS);
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) s += partials[i];
  s = wave_sum_f64(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* sumsq = reinterpret_cast<double*>(st + GC_SUMSQ);
    const double total = *sumsq + (((red[0] + red[1]) + red[2]) + red[3]);
    *sumsq = total;
    if (ls && nonfinite_f64(total)) ls[LS_FOUND_INF] = 1.f;
  }
}

extern "C" int nv_grad_sumsq(const void* grad, int grad_16bit, long count, float* clip_state, float* scale_state, int max_blocks, void* stream) {
  NV_CHECK_ARG(grad && clip_state && count > 0, "nv_grad_sumsq: null pointer / empty range");
  NV_CHECK_ARG(((uintptr_t)grad & (grad_16bit ? 1 : 3)) == 0 && ((uintptr_t)clip_state & 7) == 0, "nv_grad_sumsq: grad must be element-aligned, clip_state 8-byte aligned");
  const long per = grad_16bit ? 8 : 4;
  long blocks = (count / per + 256L * GC_UNROLL - 1) / (256L * GC_UNROLL);
  if (blocks > GC_MAX_BLOCKS) blocks = GC_MAX_BLOCKS;
  if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
  if (blocks < 1) blocks = 1;
  double* partials = reinterpret_cast<double*>(clip_state + GC_PARTIALS);
  NV_DISPATCH_OPERAND(T,
    if (grad_16bit) hipLaunchKernelGGL((grad_sumsq_kernel<true, T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, count, partials);
    else hipLaunchKernelGGL((grad_sumsq_kernel<false, T>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, count, partials));
  NV_CHECK_LAUNCH("nv_grad_sumsq");
  hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, clip_state, (int)blocks, scale_state);
  NV_CHECK_LAUNCH("nv_grad_sumsq (partials)");
  return NV_OK;
}

// clip_coef_clamped of clip_grad_norm_: fp32 arithmetic on the fp32 norm.  An infinite norm gives 0, a NaN norm NaN (the comparison
// is false, so the NaN passes - fminf would answer 1); exactly 1 whenever the quotient is >= 1.
__global__ void grad_clip_finish_kernel(float* __restrict__ st, float max_norm, float grad_scale, const float* __restrict__ ls) {
  if (threadIdx.x != 0) return;
  double* sumsq = reinterpret_cast<double*>(st + GC_SUMSQ);
  const double factor = (double)fabsf(grad_scale) * (ls ? (double)ls[LS_UNSCALE] : 1.0);
  const float total_norm = (float)(sqrt(*sumsq) * factor);
  const float c = max_norm / (total_norm + 1e-6f);
  st[GC_TOTAL_NORM] = total_norm;
  st[GC_COEF] = c > 1.f ? 1.f : c;
  *sumsq = 0.0;
}

extern "C" int nv_grad_clip_finish(float* clip_state, float max_norm, float grad_scale, const float* scale_state, void* stream) {
  NV_CHECK_ARG(clip_state && ((uintptr_t)clip_state & 7) == 0 && max_norm > 0.f && max_norm <= 3.402823466e38f, "nv_grad_clip_finish: null / misaligned state or max_norm not a finite positive number");
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, clip_state, max_norm, grad_scale, scale_state);
  NV_CHECK_LAUNCH("nv_grad_clip_finish");
  return NV_OK;
}
