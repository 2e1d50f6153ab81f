// What the evaluation kernels (features.hip, probe.hip, cls_metrics.hip, perm_test.hip, segments.hip) share: the individually rounded
// operators, the wave and four-wave sums over integers and doubles, the label rule, the walk over a segment's rows and the host's split
// rule - one definition each, so that two kernels that must agree call the same code.  The .hip files that switch contraction off do so
// AFTER their includes, which does not reach this header, so the operators carry the pragma in their own bodies.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ rounded operators
// Every fp32 / fp64 operation through these is rounded on its own.  The toolchain's rounded intrinsics (__fadd_rn ...) are inline functions
// of a header that is compiled under the default contraction mode, so a product of theirs feeding a sum of theirs still becomes a fused
// multiply-add after inlining (the probe's Adam step p - step * q did, and lost its bit-equality with the torch expressions).  These are
// defined under `contract(off)` instead, as ema.hip writes its operators.  MFMA builtins are not affected.
#define NV_ROUNDED_OP(T, name, op) \
  __device__ __forceinline__ T name(T a, T b) { _Pragma("clang fp contract(off)") return a op b; }
NV_ROUNDED_OP(float, radd, +)
NV_ROUNDED_OP(float, rsub, -)
NV_ROUNDED_OP(float, rmul, *)
NV_ROUNDED_OP(float, rdiv, /)
NV_ROUNDED_OP(double, dadd, +)
NV_ROUNDED_OP(double, dsub, -)
NV_ROUNDED_OP(double, dmul, *)
#undef NV_ROUNDED_OP

// ------------------------------------------------------------------------------------------------ sums
// The integer butterflies beside common.h's float and double ones.  They live here, not there: an int overload in sight of every source
// could change which wave_sum an existing call on the training path resolves to.
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
  return v;
}

// The sums of K values over a workgroup of four waves, behind ONE barrier: the wave butterfly, the waves' results in red[k][wave], then
// (r0 + r1) + (r2 + r3) - the one association of the double sums; integers do not care.  Every thread calls it and every thread gets the
// sums.  A second call on the same `red` needs a barrier of the caller's in between.
template <typename T, int K>
__device__ __forceinline__ void block_sum4(T (&v)[K], T (&red)[K][4]) {
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}
template <typename T>
__device__ __forceinline__ T block_sum4(T v, T (&red)[1][4]) {
  T one[1] = {v};
  block_sum4(one, red);
  return one[0];
}

// ------------------------------------------------------------------------------------------------ labels and segments
// a label outside [0, C) means: the row is not used
__device__ __forceinline__ bool valid_label(int y, int C) { return y >= 0 && y < C; }

// f(row) for the rows of segment g of the CSR (order, offsets) over N rows, in the segment's order.  The bounds are clamped and a row
// outside [0, N) is skipped: nv_segment_csr_check refuses such a table on the host; nothing is read through an unchecked index.
template <typename F>
__device__ __forceinline__ void segment_rows(const int* __restrict__ order, const int* __restrict__ offsets, int g, int N, F&& f) {
  const int b = max(offsets[g], 0), e = min(offsets[g + 1], N);
  for (int p = b; p < e; ++p) {
    const int r = order[p];
    if (r >= 0 && r < N) f(r);
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The splits of a kernel whose workgroup (x, y) walks the inner tiles of split y for outer tile x: the request, or about four workgroups
// per CU (1024) when it is 0; at most the inner tiles and max_splits; then rebalanced so that no split is empty.
static inline int nv_resolve_splits(int outer_tiles, int inner_tiles, int requested, int max_splits) {
  int s = requested > 0 ? requested : (1024 + outer_tiles - 1) / outer_tiles;
  if (s > inner_tiles) s = inner_tiles;
  if (s > max_splits) s = max_splits;
  const int tps = (inner_tiles + s - 1) / s;
  return (inner_tiles + tps - 1) / tps;
}
