// Device helpers shared by the attribution kernels (attribution.hip, perturb.hip, path_attr.hip): one definition each, so that two
// kernels that must agree bit for bit call the same code.
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
