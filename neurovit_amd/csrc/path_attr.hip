// Path attribution on the device: the steps around the forward and the data-only backward of integrated gradients
// (ViT.integrated_gradients / NeuroEncoder.integrated_gradients).  The passes are the engine's; this file writes the points of the
// straight path between a baseline and the input, turns the logits of those points into the gradient of a class score, adds the
// weighted input gradients up, and pools the finished attribution over the patches.
//
//   nv_path_points        x [B, V] + baseline + jobs [J, 2] of (b, k) + alphas [K] -> out [J, V] = bl + alphas[k] (x[b] - bl)
//   nv_class_score_grads  logits [J, C] -> dlogits [J, C]: the one-hot of the class of each job's source volume, or the gradient of its
//                         softmax probability
//   nv_path_accumulate    acc[b] += weights[k] g[j] over the jobs of volume b, in job order
//   nv_path_finish        attr = (x - bl) acc
//   nv_attr_token_sums    attr [B, S0, S1, S2] -> sums [B, N, 2]: signed sum and sum of absolute values of every patch's voxels
//
// The first, third and fourth stream dense [rows, V] buffers whose rows start at any 4-byte alignment (27^3 floats are no multiple of 16
// bytes): a workgroup owns PA_SPAN consecutive elements of one row, the 16-byte groups follow the alignment of the buffer it WRITES
// (split_span) and every other buffer is read as 16-byte vectors when its row has that alignment
// too, element by element otherwise.  Every output element is owned by one thread; there are no atomics.  The arithmetic is written
// as separately rounded fp32 operations: contraction is off for the whole file, so no product and sum below becomes an FMA.
#include "attr_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int PA_THREADS = 256;
constexpr int PA_SPAN = 4096;            // elements of one row a workgroup owns: four 16-byte groups per thread
constexpr int PP_GROUP = 8;              // jobs one workgroup of path_points_kernel serves from one read of its span of x
constexpr int AC_MAX_JOBS = 1024;        // jobs of one nv_path_accumulate call: 12 KB of LDS tables

// ------------------------------------------------------------------------------------------------ path points
// Grid (ceil(V / PA_SPAN), ceil(J / PP_GROUP)).  A workgroup owns one span of PP_GROUP consecutive jobs.  The jobs are taken in runs of
// equal source volume b (runs of one job when V is no multiple of four, since the jobs' rows then differ in alignment): x[b] and the
// baseline are read and x - bl is formed ONCE per run, then every job of the run multiplies, adds and stores.  The point buffer is
// written once and read by the next forward's patch gather only: non-temporal stores.
__global__ __launch_bounds__(PA_THREADS) void path_points_kernel(const float* __restrict__ x, int B, long V, const int* __restrict__ jobs, int J,
                                                                 const float* __restrict__ alphas, int K, float value, const float* __restrict__ base,
                                                                 long base_stride, float* __restrict__ out) {
  __shared__ int s_b[PP_GROUP];          // source volume, -1 for a job that is skipped
  __shared__ float s_a[PP_GROUP];
  const int tid = threadIdx.x;
  const int j_first = blockIdx.y * PP_GROUP, n_jobs = min(PP_GROUP, J - j_first);
  if (tid < n_jobs) {
    const int b = jobs[2L * (j_first + tid)], k = jobs[2L * (j_first + tid) + 1];
    const bool ok = b >= 0 && b < B && k >= 0 && k < K;
    s_b[tid] = ok ? b : -1;
    s_a[tid] = ok ? alphas[k] : 0.f;
  }
  __syncthreads();
  const long e0 = (long)blockIdx.x * PA_SPAN;
  const int len = (int)min((long)PA_SPAN, V - e0);
  const bool same_alignment = (V & 3) == 0;
  int r0 = 0;
  // (mask_patches_kernel of perturb.hip walks the same runs over its three-column jobs, which it validates as it goes)
  while (r0 < n_jobs) {                                    // (every condition below is uniform over the workgroup)
    const int b = s_b[r0];
    int r1 = r0 + 1;
    while (same_alignment && r1 < n_jobs && s_b[r1] == b) ++r1;
    if (b < 0) { r0 = r1; continue; }                      // such a job reads nothing and writes nothing
    const float* xp = x + (long)b * V + e0;
    const float* bp = base ? base + (long)b * base_stride + e0 : nullptr;
    const long first = (long)(j_first + r0) * V + e0;
    float* o = out + first;                                // (job r of the run: (r - r0) V further, the same alignment)
    const Span s = split_span(first, len);
    auto single = [&](int e) {
      const float bv = bp ? bp[e] : value;
      const float d = xp[e] - bv;
      for (int r = r0; r < r1; ++r) {
        const float t = s_a[r] * d;
        o[(long)(r - r0) * V + e] = bv + t;
      }
    };
    for (int e = tid; e < s.head; e += PA_THREADS) single(e);
    for (int e = s.tail + tid; e < len; e += PA_THREADS) single(e);
    const bool x_vec = is_aligned16(xp + s.head), b_vec = bp && is_aligned16(bp + s.head);
    for (int g = tid; g < s.groups; g += PA_THREADS) {
      const int e = s.head + 4 * g;
      const f32x4 xv = load4(xp + e, x_vec);
      const f32x4 bv = bp ? load4(bp + e, b_vec) : f32x4{value, value, value, value};
      const f32x4 d = xv - bv;
      for (int r = r0; r < r1; ++r) {
        const f32x4 t = s_a[r] * d;
        __builtin_nontemporal_store(bv + t, reinterpret_cast<f32x4*>(o + (long)(r - r0) * V + e));
      }
    }
    r0 = r1;
  }
}

// ------------------------------------------------------------------------------------------------ gradient of the class score
constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;

// One wave per job.  kind 1: the one-hot of the class.  kind 0: p_c (delta_ci - p_i) with p = exp(l - max) / sum exp(l - max) in fp32
// (wave_softmax_stats: the statistics nv_class_scores divides by).
// A job whose source volume is outside [0, B) writes nothing; a class outside [0, C) gives a row of NaN.
__global__ __launch_bounds__(CS_THREADS) void class_score_grads_kernel(const float* __restrict__ logits, int J, int C, const int* __restrict__ jobs,
                                                                       const long* __restrict__ cls, int B, int kind, float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
  if (j >= J) return;
  const int b = jobs[2L * j];
  if (b < 0 || b >= B) return;
  const long c = cls[b];
  const float* row = logits + (long)j * C;
  float* drow = dlogits + (long)j * C;
  if (c < 0 || c >= C) {
    for (int i = lane; i < C; i += 64) drow[i] = __uint_as_float(0x7fc00000u);
    return;
  }
  if (kind == 1) {
    for (int i = lane; i < C; i += 64) drow[i] = (i == c) ? 1.f : 0.f;
    return;
  }
  float mx, sum;
  wave_softmax_stats(row, C, lane, mx, sum);
  const float pc = expf(row[c] - mx) / sum;
  for (int i = lane; i < C; i += 64) {
    const float pi = expf(row[i] - mx) / sum;
    drow[i] = pc * (((i == c) ? 1.f : 0.f) - pi);
  }
}

// ------------------------------------------------------------------------------------------------ weighted sum of the input gradients
// Grid (ceil(V / PA_SPAN), B).  A workgroup owns one span of acc[b]: it lists the jobs of volume b in job order (flags by all threads,
// compacted by one), leaves at once when there are none, and otherwise reads its span of acc[b], adds w_k g[j] job after job and
// stores it: acc is read and written once per call whatever the number of jobs.
__global__ __launch_bounds__(PA_THREADS) void path_accumulate_kernel(const float* __restrict__ g, const int* __restrict__ jobs, int J,
                                                                     const float* __restrict__ weights, int K, float* __restrict__ acc, long V) {
  __shared__ int s_k[AC_MAX_JOBS];       // step index of job j when it belongs to this volume, else -1
  __shared__ int s_j[AC_MAX_JOBS];       // the volume's jobs, in job order
  __shared__ float s_w[AC_MAX_JOBS];
  __shared__ int s_n;
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int j = tid; j < J; j += PA_THREADS) {
    const int jb = jobs[2L * j], k = jobs[2L * j + 1];
    s_k[j] = (jb == b && k >= 0 && k < K) ? k : -1;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < J; ++j)
      if (s_k[j] >= 0) { s_j[n] = j; s_w[n] = weights[s_k[j]]; ++n; }
    s_n = n;
  }
  __syncthreads();
  const int n = s_n;
  if (n == 0) return;                                      // a volume absent from the jobs is not touched
  const long e0 = (long)blockIdx.x * PA_SPAN;
  const int len = (int)min((long)PA_SPAN, V - e0);
  const long first = (long)b * V + e0;
  float* a = acc + first;
  const float* g0 = g + e0;
  const Span s = split_span(first, len);
  auto single = [&](int e) {
    float v = a[e];
    for (int i = 0; i < n; ++i) {
      const float t = s_w[i] * g0[(long)s_j[i] * V + e];
      v = v + t;
    }
    a[e] = v;
  };
  for (int e = tid; e < s.head; e += PA_THREADS) single(e);
  for (int e = s.tail + tid; e < len; e += PA_THREADS) single(e);
  for (int q = tid; q < s.groups; q += PA_THREADS) {
    const int e = s.head + 4 * q;
    f32x4 v = *reinterpret_cast<const f32x4*>(a + e);
    for (int i = 0; i < n; ++i) {
      const float* gp = g0 + (long)s_j[i] * V + e;         // (its alignment is the same for every group of the span: a uniform branch)
      const f32x4 t = s_w[i] * load4(gp, is_aligned16(gp));
      v = v + t;
    }
    *reinterpret_cast<f32x4*>(a + e) = v;
  }
}

// ------------------------------------------------------------------------------------------------ attribution
// Grid (ceil(V / PA_SPAN), B): attr[b] = (x[b] - bl) acc[b] over one span.
__global__ __launch_bounds__(PA_THREADS) void path_finish_kernel(const float* __restrict__ acc, const float* __restrict__ x, long V, float value,
                                                                 const float* __restrict__ base, long base_stride, float* __restrict__ attr) {
  const int tid = threadIdx.x, b = blockIdx.y;
  const long e0 = (long)blockIdx.x * PA_SPAN;
  const int len = (int)min((long)PA_SPAN, V - e0);
  const long first = (long)b * V + e0;
  const float* ap = acc + first;
  const float* xp = x + first;
  const float* bp = base ? base + (long)b * base_stride + e0 : nullptr;
  float* o = attr + first;
  const Span s = split_span(first, len);
  auto single = [&](int e) {
    const float d = xp[e] - (bp ? bp[e] : value);
    o[e] = d * ap[e];
  };
  for (int e = tid; e < s.head; e += PA_THREADS) single(e);
  for (int e = s.tail + tid; e < len; e += PA_THREADS) single(e);
  const bool a_vec = is_aligned16(ap + s.head), x_vec = is_aligned16(xp + s.head), b_vec = bp && is_aligned16(bp + s.head);
  for (int q = tid; q < s.groups; q += PA_THREADS) {
    const int e = s.head + 4 * q;
    const f32x4 bv = bp ? load4(bp + e, b_vec) : f32x4{value, value, value, value};
    const f32x4 d = load4(xp + e, x_vec) - bv;
    *reinterpret_cast<f32x4*>(o + e) = d * load4(ap + e, a_vec);
  }
}

// ------------------------------------------------------------------------------------------------ patch sums
// One wave per (volume, token).  Token t = c2 G0 G1 + c0 G1 + c1 holds the voxels (c0 p0 + d0, c1 p1 + d1, c2 p2 + d2); lane l adds the
// voxels q = l, l + 64, .. of the patch (q = (d0 p1 + d1) p2 + d2) in double, and a six-level butterfly adds the 64 partials: a fixed
// order, the same bits on every run.  The attribution was written a moment ago and is 1 / K of the bytes the path moved: the p2-float
// runs are read as they lie.
__global__ __launch_bounds__(CS_THREADS) void attr_token_sums_kernel(const float* __restrict__ attr, int S0, int S1, int S2, int p0, int p1, int p2,
                                                                     long tokens, float* __restrict__ sums) {
  const int lane = threadIdx.x & 63;
  const long tok = (long)blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
  if (tok >= tokens) return;
  const int G0 = S0 / p0, G1 = S1 / p1, G2 = S2 / p2, N = G0 * G1 * G2;
  const long b = tok / N;
  const int t = (int)(tok - b * N);
  const int c2 = t / (G0 * G1), c0 = (t / G1) % G0, c1 = t % G1;
  const float* p = attr + b * ((long)S0 * S1 * S2) + ((long)(c0 * p0) * S1 + c1 * p1) * S2 + c2 * p2;
  const int P = p0 * p1 * p2;
  double sum = 0.0, mag = 0.0;
  for (int q = lane; q < P; q += 64) {
    const int r = q / p2, d2 = q - r * p2, d0 = r / p1, d1 = r - d0 * p1;
    const double v = (double)p[((long)d0 * S1 + d1) * S2 + d2];
    sum += v;
    mag += fabs(v);
  }
  sum = wave_sum(sum);
  mag = wave_sum(mag);
  if (lane == 0) {
    sums[2 * tok] = (float)sum;
    sums[2 * tok + 1] = (float)mag;
  }
}
}  // namespace

extern "C" int nv_path_points(const float* x, int B, long V, const int* jobs, int J, const float* alphas, int K, float value, const float* base,
                              long base_stride, float* out, void* stream) {
  NV_CHECK_ARG(x && jobs && alphas && out && B > 0 && V > 0 && J > 0 && K > 0, "nv_path_points: bad arguments (null pointer, or B / V / J / K not positive)");
  const long spans = (V + PA_SPAN - 1) / PA_SPAN, job_groups = ((long)J + PP_GROUP - 1) / PP_GROUP;
  NV_CHECK_ARG(spans < (1L << 31) && job_groups <= 65535, "nv_path_points: %ld elements per volume or %d jobs beyond one launch (at most %d jobs)", V, J,
               65535 * PP_GROUP);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned(x, 4) && nv_aligned(base, 4) && nv_aligned(jobs, 4) && nv_aligned(alphas, 4),
               "nv_path_points: out 16-byte aligned, every other buffer 4-byte aligned");
  NV_CHECK_ARG(base_stride == 0 || base_stride >= V, "nv_path_points: baseline stride %ld is neither 0 nor at least one volume", base_stride);
  hipLaunchKernelGGL(path_points_kernel, dim3((unsigned)spans, (unsigned)job_groups), dim3(PA_THREADS), 0, (hipStream_t)stream, x, B, V, jobs, J, alphas, K,
                     value, base, base_stride, out);
  NV_CHECK_LAUNCH("nv_path_points");
  return NV_OK;
}

extern "C" int nv_class_score_grads(const float* logits, int J, int C, const int* jobs, const long* cls, int B, int kind, float* dlogits, void* stream) {
  NV_CHECK_ARG(logits && jobs && cls && dlogits && J > 0 && C > 0 && B > 0, "nv_class_score_grads: bad arguments (null pointer, or J / C / B not positive)");
  NV_CHECK_ARG(kind == NV_SCORE_PROB || kind == NV_SCORE_LOGIT, "nv_class_score_grads: kind %d is neither NV_SCORE_PROB nor NV_SCORE_LOGIT", kind);
  NV_CHECK_ARG(nv_aligned(logits, 4) && nv_aligned(jobs, 4) && nv_aligned(cls, 8) && nv_aligned(dlogits, 4), "nv_class_score_grads: element-aligned buffers");
  hipLaunchKernelGGL(class_score_grads_kernel, dim3((J + CS_WAVES - 1) / CS_WAVES), dim3(CS_THREADS), 0, (hipStream_t)stream, logits, J, C, jobs, cls, B,
                     kind, dlogits);
  NV_CHECK_LAUNCH("nv_class_score_grads");
  return NV_OK;
}

extern "C" int nv_path_accumulate(const float* g, const int* jobs, int J, const float* weights, int K, float* acc, int B, long V, void* stream) {
  NV_CHECK_ARG(g && jobs && weights && acc && J > 0 && K > 0 && B > 0 && V > 0, "nv_path_accumulate: bad arguments (null pointer, or J / K / B / V not positive)");
  NV_CHECK_ARG(J <= AC_MAX_JOBS, "nv_path_accumulate: %d jobs, at most %d in one call", J, AC_MAX_JOBS);
  const long spans = (V + PA_SPAN - 1) / PA_SPAN;
  NV_CHECK_ARG(spans < (1L << 31) && B <= 65535, "nv_path_accumulate: %ld elements per volume or %d volumes beyond one launch (at most 65535 volumes)", V, B);
  NV_CHECK_ARG(nv_aligned16(acc) && nv_aligned(g, 4) && nv_aligned(jobs, 4) && nv_aligned(weights, 4),
               "nv_path_accumulate: acc 16-byte aligned, every other buffer 4-byte aligned");
  hipLaunchKernelGGL(path_accumulate_kernel, dim3((unsigned)spans, (unsigned)B), dim3(PA_THREADS), 0, (hipStream_t)stream, g, jobs, J, weights, K, acc, V);
  NV_CHECK_LAUNCH("nv_path_accumulate");
  return NV_OK;
}

extern "C" int nv_path_finish(const float* acc, const float* x, int B, long V, float value, const float* base, long base_stride, float* attr, void* stream) {
  NV_CHECK_ARG(acc && x && attr && B > 0 && V > 0, "nv_path_finish: bad arguments (null pointer, or B / V not positive)");
  const long spans = (V + PA_SPAN - 1) / PA_SPAN;
  NV_CHECK_ARG(spans < (1L << 31) && B <= 65535, "nv_path_finish: %ld elements per volume or %d volumes beyond one launch (at most 65535 volumes)", V, B);
  NV_CHECK_ARG(nv_aligned16(attr) && nv_aligned(acc, 4) && nv_aligned(x, 4) && nv_aligned(base, 4), "nv_path_finish: attr 16-byte aligned, every other buffer 4-byte aligned");
  NV_CHECK_ARG(base_stride == 0 || base_stride >= V, "nv_path_finish: baseline stride %ld is neither 0 nor at least one volume", base_stride);
  hipLaunchKernelGGL(path_finish_kernel, dim3((unsigned)spans, (unsigned)B), dim3(PA_THREADS), 0, (hipStream_t)stream, acc, x, V, value, base, base_stride, attr);
  NV_CHECK_LAUNCH("nv_path_finish");
  return NV_OK;
}

extern "C" int nv_attr_token_sums(const float* attr, int B, const int* size3, const int* patch3, float* sums, void* stream) {
  NV_CHECK_ARG(attr && size3 && patch3 && sums && B > 0, "nv_attr_token_sums: bad arguments (null pointer, or B not positive)");
  const int S0 = size3[0], S1 = size3[1], S2 = size3[2], p0 = patch3[0], p1 = patch3[1], p2 = patch3[2];
  NV_CHECK_ARG(S0 > 0 && S1 > 0 && S2 > 0 && p0 > 0 && p1 > 0 && p2 > 0, "nv_attr_token_sums: volume and patch extents must be positive");
  NV_CHECK_ARG(S0 % p0 == 0 && S1 % p1 == 0 && S2 % p2 == 0, "nv_attr_token_sums: volume %d x %d x %d is not a whole number of %d x %d x %d patches", S0, S1,
               S2, p0, p1, p2);
  const long N = (long)(S0 / p0) * (S1 / p1) * (S2 / p2), P = (long)p0 * p1 * p2, tokens = (long)B * N;
  NV_CHECK_ARG(N < (1L << 31) && P < (1L << 31) && (tokens + CS_WAVES - 1) / CS_WAVES < (1L << 31),
               "nv_attr_token_sums: %ld patches of %ld voxels in %d volumes beyond one launch", N, P, B);
  NV_CHECK_ARG(nv_aligned(attr, 4) && nv_aligned(sums, 4), "nv_attr_token_sums: element-aligned buffers");
  hipLaunchKernelGGL(attr_token_sums_kernel, dim3((unsigned)((tokens + CS_WAVES - 1) / CS_WAVES)), dim3(CS_THREADS), 0, (hipStream_t)stream, attr, S0, S1, S2, p0,
                     p1, p2, tokens, sums);
  NV_CHECK_LAUNCH("nv_attr_token_sums");
  return NV_OK;
}
