// Device helpers shared by the attribution kernels (attribution.hip, series_attr.hip, perturb.hip, path_attr.hip): one definition each,
// so that two kernels that must agree bit for bit call the same code.
#pragma once
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
template <typename E> using vec4 = E __attribute__((ext_vector_type(4)));      // vec4<float> is f32x4, vec4<unsigned> is u32x4

// ---- streaming a span of a row that starts at any 4-byte alignment: the elements in front of the first 16-byte group of the buffer
// that is WRITTEN are handled singly ([0, head)), then `groups` groups of four from `head`, then the rest singly ([tail, len))
struct Span { int head, groups, tail; };

// `first`: flat element offset of the span's first element from the 16-byte aligned base of the buffer that is written
__device__ __forceinline__ Span split_span(long first, int len) {
  int head = (int)((4 - (first & 3)) & 3);
  if (head > len) head = len;
  const int groups = (len - head) >> 2;
  return Span{head, groups, head + 4 * groups};
}
__device__ __forceinline__ bool is_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// four consecutive elements: one 16-byte load when the caller found `p` aligned (uniform per span), element by element otherwise
template <typename E>
__device__ __forceinline__ vec4<E> load4(const E* p, bool vec) {
  if (vec) return *reinterpret_cast<const vec4<E>*>(p);
  return vec4<E>{p[0], p[1], p[2], p[3]};
}

// ---- order-preserving map of the fp32 bit patterns onto unsigned integers (and back); -0.0 sorts below +0.0, no finite value has key 0
__device__ __forceinline__ unsigned float_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of_key(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- softmax statistics of one row of C logits by one wave: mx = max_i row[i], sum = sum_i exp(row[i] - mx) in fp32 with the library
// expf; a lane-strided partial per lane and a six-level butterfly, so a row of C <= 64 classes adds each term once in a balanced
// tree.  Every lane returns both.  nv_class_scores and nv_class_score_grads call it: integrated gradients' completeness check compares
// the scores of the one with the gradients of the other.  Contraction is off inside, so it compiles the same in every file.
__device__ __forceinline__ void wave_softmax_stats(const float* __restrict__ row, int C, int lane, float& mx, float& sum) {
#pragma clang fp contract(off)
  mx = -INFINITY;
  for (int i = lane; i < C; i += 64) mx = fmaxf(mx, row[i]);
  mx = wave_max(mx);
  sum = 0.f;
  for (int i = lane; i < C; i += 64) sum += expf(row[i] - mx);
  sum = wave_sum(sum);
}

// ---- token maps -> thresholded maps: the selection shared by nv_token_map_to_volume (one workgroup per volume, attribution.hip) and
// nv_series_map_to_volumes (one workgroup per sample over its T volumes, series_attr.hip)
// The k-th smallest (0-based) of keys[0, N): radix select, eight bits per pass.  Every thread of the workgroup of THREADS (>= 256)
// threads calls it and gets the key.  hist: 256 bins, s_sel: 2 words, both in LDS.
template <int THREADS>
__device__ unsigned select_kth(const unsigned* keys, int N, int k, unsigned* hist, unsigned* s_sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0, mask = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += THREADS) {
      const unsigned key = keys[i];
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {                                        // one wave: lane l owns bins 4l .. 4l + 3
      const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
      const unsigned mine = c0 + c1 + c2 + c3;
      unsigned incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const unsigned excl = incl - mine, kk = (unsigned)k;
      if (excl <= kk && kk < incl) {                       // exactly one lane: the counts of the surviving keys sum to more than k
        unsigned bin = 4 * lane, below = excl;
        if (kk >= below + c0) { below += c0; ++bin;
          if (kk >= below + c1) { below += c1; ++bin;
            if (kk >= below + c2) { below += c2; ++bin; } } }
        s_sel[0] = bin; s_sel[1] = kk - below;
      }
    }
    __syncthreads();
    prefix |= s_sel[0] << shift; mask |= 255u << shift;
    k = (int)s_sel[1];
    __syncthreads();                                       // s_sel and hist are rewritten by the next pass
  }
  return prefix;
}

// The position q (N - 1) of the quantile among the N order statistics, as torch.quantile: split on the host in double.
struct QuantilePos { int i_lo, i_hi; double w; };
static inline QuantilePos quantile_pos(double keep_percent, long N) {
  const double q = 1.0 - keep_percent / 100.0, pos = q * (double)(N - 1);
  int i_lo = (int)floor(pos);
  if (i_lo > N - 1) i_lo = (int)N - 1;
  const int i_hi = i_lo + 1 < N ? i_lo + 1 : (int)N - 1;
  return QuantilePos{i_lo, i_hi, pos - (double)i_lo};
}

// LDS scratch of threshold_block beside the keys
struct ThresholdScratch { unsigned hist[256]; float red[2 * 16]; unsigned sel[2], cnt, next; };

// One workgroup of THREADS threads turns the N cells maps[0, N) into norm[0, N) (min-max normalised over the N cells when `normalize`),
// sparse[0, N) (the same with the cells under the cut zeroed) and returns the cut (every thread): the quantile of position `pos` by
// torch.quantile's linear rule.  keys: N words of LDS.
template <int THREADS>
__device__ float threshold_block(const float* __restrict__ maps, int N, int normalize, QuantilePos pos, float* __restrict__ norm,
                                 float* __restrict__ sparse, unsigned* keys, ThresholdScratch& s) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float lo = INFINITY, hi = -INFINITY;
  if (normalize) {
    for (int i = tid; i < N; i += THREADS) { const float v = maps[i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane == 0) { s.red[2 * wid] = lo; s.red[2 * wid + 1] = hi; }
    __syncthreads();
    lo = s.red[0]; hi = s.red[1];
    for (int v = 1; v < THREADS / 64; ++v) { lo = fminf(lo, s.red[2 * v]); hi = fmaxf(hi, s.red[2 * v + 1]); }
  }
  const float inv = 1.0f / (hi - lo + 1e-8f);
  for (int i = tid; i < N; i += THREADS) {
    float v = maps[i];
    if (normalize) v = (v - lo) * inv;
    norm[i] = v;
    keys[i] = float_key(v);
  }
  if (tid == 0) { s.cnt = 0; s.next = 0xffffffffu; }
  __syncthreads();
  const unsigned k_lo = select_kth<THREADS>(keys, N, pos.i_lo, s.hist, s.sel);
  unsigned k_hi = k_lo;
  if (pos.i_hi != pos.i_lo) {                              // the next order statistic: k_lo again if it repeats, else the smallest key above it
    unsigned cnt = 0, nxt = 0xffffffffu;
    for (int i = tid; i < N; i += THREADS) {
      const unsigned key = keys[i];
      if (key <= k_lo) ++cnt; else nxt = min(nxt, key);
    }
    atomicAdd(&s.cnt, cnt); atomicMin(&s.next, nxt);
    __syncthreads();
    k_hi = ((int)s.cnt > pos.i_hi) ? k_lo : s.next;
  }
  // torch.quantile(interpolation='linear') = lerp(s[lo], s[hi], w) in double (ATen's lerp: two forms around w = 0.5), rounded to fp32
  float cut;
  {
#pragma clang fp contract(off)
    const double w = pos.w, a = (double)float_of_key(k_lo), e = (double)float_of_key(k_hi);
    const double c = (w < 0.5) ? a + w * (e - a) : e - (e - a) * (1.0 - w);
    cut = (float)c;
  }
  for (int i = tid; i < N; i += THREADS) {
    const float v = float_of_key(keys[i]);
    sparse[i] = (v >= cut) ? v : 0.f;
  }
  return cut;
}

// ---- trilinear upsampling (align_corners = False): the taps of one output index and the two-term blend every lerp is written as
struct AxisTap { int i0, i1; float l0, l1; };

// ATen's area_pixel_compute_source_index (align_corners = False) and linear taps of one output index; scale = (float)G / S
__device__ __forceinline__ AxisTap axis_tap(int dst, float scale, int G) {
#pragma clang fp contract(off)
  AxisTap t;
  const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  t.i0 = min((int)src, G - 1);
  t.i1 = min(t.i0 + 1, G - 1);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.0f - t.l1;
  return t;
}
// the packed taps of the y and z tables: i0 | i1 << 16 (the row taps premultiplied by the row length) and lambda1
__device__ __forceinline__ void fill_axis_table(int* idx, float* lam, int S, float scale, int G, int mul, int tid, int threads) {
  for (int i = tid; i < S; i += threads) { const AxisTap t = axis_tap(i, scale, G); idx[i] = (t.i0 * mul) | ((t.i1 * mul) << 16); lam[i] = t.l1; }
}
// l0 a + l1 b with its rounding spelled out: the product l1 b rounded, then ONE fused multiply-add.  Left to the compiler, which of the
// two products is fused differs from kernel to kernel and even between the scalar and the 16-byte paths of one kernel (a last-bit
// difference); spelled out, every kernel that calls it gives an output the same bits at any alignment, in any layout.
__device__ __forceinline__ float blend(float l0, float a, float l1, float b) {
#pragma clang fp contract(off)
  const float second = l1 * b;
  return __builtin_fmaf(l0, a, second);
}
// one output from the four cells (r0 | r1, c0 | c1) of a plane whose cell (r, c) lies at plane[(r + c) * step]: the z lerps, then the y lerp
__device__ __forceinline__ float plane_value(const float* plane, int step, int yy, float ly1, int zz, float lz1) {
  const float ly0 = 1.0f - ly1, lz0 = 1.0f - lz1;
  const int r0 = yy & 0xffff, r1 = yy >> 16, c0 = zz & 0xffff, c1 = zz >> 16;
  const float a = blend(lz0, plane[(r0 + c0) * step], lz1, plane[(r0 + c1) * step]);
  const float c = blend(lz0, plane[(r1 + c0) * step], lz1, plane[(r1 + c1) * step]);
  return blend(ly0, a, ly1, c);
}

// ---- host launchers of attribution.hip's kernels that series_attr.hip's entry points reuse (the arguments arrive checked)
int nv_attr_gc_blocks(long rows, int groups);               // workgroups per group of the Grad-CAM reduction
long nv_attr_gc_workspace_bytes(int groups, int blocks);
int nv_attr_gradcam_launch(const char* name, const void* act, const float* grad, int n, int d, int groups, int R, int blocks, float* cam, float* minmax,
                           void* workspace, void* stream);
// V volumes of N <= 4096 cells, every volume on its own: norm / sparse [V, N], cuts [V]
int nv_attr_threshold_launch(const char* name, const float* maps, int V, int N, int normalize, double keep_percent, float* norm, float* sparse, float* cuts,
                             void* stream);
// sparse [V, G0, G1, G2] -> out [V, S0, S1, S2]
int nv_attr_upsample_launch(const char* name, const float* sparse, int V, const int* grid3, const int* out3, float* out, void* stream);
