// Shared pieces of the kernels that recompute attention probabilities from a layer's qkv buffer: attn_probs.hip (the forward export) and
// attn_grad.hip (the gradient w.r.t. the probabilities and the class-specific relevance).  Both must form a probability with the SAME
// bits - same MFMA order, same row statistics, same exp2 expression - so the fragment loads, the score tile, the statistics sweep and the
// transposed store live here once.
#pragma once
#include "common.h"

namespace {

constexpr int PR_MAXH = 64;              // heads of a fused 16-bit launch (LDS row statistics)
constexpr int PR_LD = 68;                // LDS row pitch of the transposed tile, floats (272 B: rows stay 16-byte aligned)
constexpr int PR_WAVES = 4;              // waves of a workgroup: they share its query rows and split the keys
constexpr float PR_LOG2E = 1.44269504088896340736f;

// (m, l) of two partial row sweeps in the exp2 domain: m = max, l = sum of exp2(u - m); m = -inf marks an empty sweep
__device__ __forceinline__ void pr_merge(float& m, float& l, float mo, float lo) {
  const float mn = fmaxf(m, mo);
  const float a = (m == -INFINITY) ? 0.f : l * __builtin_amdgcn_exp2f(m - mn);
  const float b = (mo == -INFINITY) ? 0.f : lo * __builtin_amdgcn_exp2f(mo - mn);
  l = a + b;
  m = mn;
}

// the tile a wave transposes through is its own: its LDS writes must land before its reads (and the reads before the next writes);
// waves of one workgroup may run different numbers of chunks, so no workgroup barrier here
__device__ __forceinline__ void wave_lds_order() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Q fragments of row tile t: lane (row l & 15, k 8 (l >> 4) .. + 8) of the 16 x 32 A operand, zero outside [0, rows) x [0, dh)
template <int KK, int RT>
__device__ __forceinline__ void pr_load_q(r16x8 (&qf)[RT][KK], const r16* __restrict__ base, long ld, int i0, int rows, int col0, int dh, int lane) {
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int i = i0 + 16 * t + (lane & 15);
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      const int k = 32 * kk + 8 * (lane >> 4);
      qf[t][kk] = (i < rows && k < dh) ? *reinterpret_cast<const r16x8*>(base + (long)i * ld + col0 + k) : r16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
}

// S of the RT row tiles against keys j0 .. j0 + 15: C fragment (row 4 (l >> 4) + r, key j0 + (l & 15)); keys >= n read as zero
template <typename T, int KK, int RT>
__device__ __forceinline__ void pr_scores(f32x4 (&s)[RT], const r16x8 (&qf)[RT][KK], const r16* __restrict__ base, long ld, int n, int j0, int kcol,
                                          int dh, int lane) {
  const int j = j0 + (lane & 15);
#pragma unroll
  for (int t = 0; t < RT; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < KK; ++kk) {
    const int k = 32 * kk + 8 * (lane >> 4);
    const r16x8 kf = (j < n && k < dh) ? *reinterpret_cast<const r16x8*>(base + (long)j * ld + kcol + k) : r16x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < RT; ++t) s[t] = mfma16<T>(qf[t][kk], kf, s[t]);
  }
}

// Row statistics of one head for the workgroup's 16 RT query rows (qf): wave wv sweeps the 16-key blocks wv, wv + 4, ... once for each
// row's max and sum (online, merged across the 16 lanes of a row group), the four partial statistics are merged through LDS in wave
// order - every workgroup, every form, every kernel: the same bits.  mrow = max of s c, irow = 1 / sum of exp2(s c - mrow).
// Contains one workgroup barrier; the caller places another before sPart is rewritten.
template <typename T, int KK, int RT>
__device__ __forceinline__ void pr_row_stats(float (&mrow)[RT][4], float (&irow)[RT][4], const r16x8 (&qf)[RT][KK], const r16* __restrict__ base, long ld,
                                             int n, int kcol, int dh, float c, float (&sPart)[PR_WAVES][16 * RT][2], int lane, int wv) {
  const int g = lane >> 4;
  f32x4 s[RT];
  float m[RT][4], l[RT][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[t][r] = -INFINITY; l[t][r] = 0.f; }
  for (int j0 = 16 * wv; j0 < n; j0 += 16 * PR_WAVES) {
    pr_scores<T, KK, RT>(s, qf, base, ld, n, j0, kcol, dh, lane);
    if (j0 + (lane & 15) < n) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float u = s[t][r] * c;
          if (u > m[t][r]) { l[t][r] = (m[t][r] == -INFINITY) ? 0.f : l[t][r] * __builtin_amdgcn_exp2f(m[t][r] - u); m[t][r] = u; }
          l[t][r] += __builtin_amdgcn_exp2f(u - m[t][r]);
        }
    }
  }
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) pr_merge(m[t][r], l[t][r], __shfl_xor(m[t][r], o, 64), __shfl_xor(l[t][r], o, 64));
      if ((lane & 15) == 0) { sPart[wv][16 * t + 4 * g + r][0] = m[t][r]; sPart[wv][16 * t + 4 * g + r][1] = l[t][r]; }
    }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * t + 4 * g + r;
      float mm = sPart[0][row][0], ll = sPart[0][row][1];
#pragma unroll
      for (int w = 1; w < PR_WAVES; ++w) pr_merge(mm, ll, sPart[w][row][0], sPart[w][row][1]);
      mrow[t][r] = mm;
      irow[t][r] = 1.0f / ll;
    }
}

// the probability of one score: the one expression every form uses
__device__ __forceinline__ float pr_prob(float s, float c, float mrow, float irow) { return __builtin_amdgcn_exp2f(s * c - mrow) * irow; }

// A wave's [16 RT rows][64 keys] tile (written in C-fragment order: tile[16 t + 4 g + r][16 kb + (lane & 15)]) out to rows i0 .. of a
// row-major [rows, n] fp32 matrix, keys j0 .. j0 + 63: every store instruction writes whole runs of a row.
__device__ __forceinline__ void pr_store_tile(float (*tile)[PR_LD], float* __restrict__ obase, int n, int i0, int valid_rows, int j0, int vec4, int lane) {
  wave_lds_order();
  if (vec4) {                          // n % 4 == 0: 16 lanes write one row's 64 keys as float4, four rows per instruction
    const int jj = j0 + 4 * (lane & 15);
    for (int rr = lane >> 4; rr < valid_rows; rr += 4)
      if (jj < n) *reinterpret_cast<float4*>(obase + (long)(i0 + rr) * n + jj) = *reinterpret_cast<const float4*>(&tile[rr][4 * (lane & 15)]);
  } else {                             // odd n: one row's 64 keys per instruction
    const int jj = j0 + lane;
    if (jj < n)
      for (int rr = 0; rr < valid_rows; ++rr) obase[(long)(i0 + rr) * n + jj] = tile[rr][lane];
  }
  wave_lds_order();
}

}  // namespace
