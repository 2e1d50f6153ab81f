// Gradient of the loss w.r.t. the attention probabilities, and the class-specific attention relevance built from it (explainability:
// what a backward hook on the reference's `attend`, or `attn.register_hook`, delivers - vit_3d.py:54-57; Chefer et al., "Generic
// Attention-model Explainability": A_l = mean_h (grad A_l * A_l)^+, R <- R + A_l R).
//
// The flash-style attention backward forms dP = dO V^T tile by tile and never stores it.  These kernels recompute it from the buffers that
// are live right behind a layer's attention backward: the layer's qkv and dAO, the 16-bit gradient of the attention output.
//
//   attn_grad16_kernel   per head:   dP[B, heads, n, n] = dO_h V_h^T - one v_mfma_f32_16x16x32 product, fp32 accumulation, no
//                                    probabilities.  Zero rows of dO give exact zero rows.
//                        relevance:  A[B, n, n] = (1 / heads) sum_h max(dP_h * P_h, 0): the workgroup walks every head of its row tile.
//                                    P_h is recomputed by attn_probs.h - the statistics sweep, score tile and exp2 expression of
//                                    nv_attn_probs, so the P used here is bit-identical to the forward export.
//                        Workgroup shape, key splits and the LDS transpose of the fp32 store are those of attn_probs16_kernel: the kernel
//                        is bound by its stores in the per-head form, by its two MFMA products over all heads in the relevance form.
//   relevance_gemv       u <- u + u A_l from the last layer down (the row-vector form of R <- R + A_l R read at the row of the token the
//                        head sees): a batched GEMV per layer, memory-bound, no [n, n] product; the first step of the cls start reads
//                        one row only.
#include "attn_probs.h"

namespace {

// grid (ceil(n / (16 RT)), B * heads [per head] or B [relevance], KS), four waves; wave w of key split z writes the 64-key chunks
// 4 z + w, + 4 KS, ...  qkv [B * n, ld] (q | k | v, each heads * dh wide), dout [B * n, ldo] (heads * dh wide); out fp32 contiguous.
template <typename T, int KK, int RT, int FORM>
__global__ __launch_bounds__(64 * PR_WAVES) void attn_grad16_kernel(const r16* __restrict__ qkv, long ld, const r16* __restrict__ dout, long ldo, int n,
                                                                    int heads, int dh, float c, float* __restrict__ out, int vec4) {
  constexpr bool REL = FORM == NV_ATTN_GRAD_RELEVANCE;
  __shared__ __attribute__((aligned(16))) float sT[PR_WAVES][16 * RT][PR_LD];
  __shared__ float sPart[PR_WAVES][16 * RT][2];
  __shared__ float sSt[REL ? PR_MAXH : 1][16 * RT][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, i0 = blockIdx.x * 16 * RT;
  const int inner = heads * dh;
  int b, h0, h1;
  if (!REL) { b = blockIdx.y / heads; h0 = blockIdx.y - b * heads; h1 = h0 + 1; }
  else { b = blockIdx.y; h0 = 0; h1 = heads; }
  const r16* base = qkv + (long)b * n * ld;
  const r16* dbase = dout + (long)b * n * ldo;
  float* obase = out + (long)blockIdx.y * n * n;
  r16x8 qf[RT][KK], gf[RT][KK];           // Q and dO fragments of the workgroup's rows
  f32x4 s[RT], dp[RT];
  float mrow[RT][4], irow[RT][4];

  if (REL) {                               // ---- pass 1: the row statistics of nv_attn_probs, every head
    for (int h = h0; h < h1; ++h) {
      pr_load_q<KK, RT>(qf, base, ld, i0, n, h * dh, dh, lane);
      pr_row_stats<T, KK, RT>(mrow, irow, qf, base, ld, n, inner + h * dh, dh, c, sPart, lane, wv);
      if (wv == 0 && (lane & 15) == 0) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) { sSt[h][16 * t + 4 * g + r][0] = mrow[t][r]; sSt[h][16 * t + 4 * g + r][1] = irow[t][r]; }
      }
      __syncthreads();                     // sPart is rewritten by the next head
    }
  } else {
    pr_load_q<KK, RT>(gf, dbase, ldo, i0, n, h0 * dh, dh, lane);
  }

  // ---- pass 2: 64 keys at a time: dP (times P, clamped, summed over the heads), transposed through LDS, stored as row runs
  const int valid_rows = min(16 * RT, n - i0);
  for (int j0 = 64 * (PR_WAVES * blockIdx.z + wv); j0 < n; j0 += 64 * PR_WAVES * gridDim.z) {
    float acc[RT][4][4];
    for (int h = h0; h < h1; ++h) {
      if (REL) {
        pr_load_q<KK, RT>(qf, base, ld, i0, n, h * dh, dh, lane);
        pr_load_q<KK, RT>(gf, dbase, ldo, i0, n, h * dh, dh, lane);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) { mrow[t][r] = sSt[h][16 * t + 4 * g + r][0]; irow[t][r] = sSt[h][16 * t + 4 * g + r][1]; }
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (j0 + 16 * kb >= n) break;                                   // wave-uniform
        pr_scores<T, KK, RT>(dp, gf, base, ld, n, j0 + 16 * kb, 2 * inner + h * dh, dh, lane);      // dO_h V_h^T
        if (REL) pr_scores<T, KK, RT>(s, qf, base, ld, n, j0 + 16 * kb, inner + h * dh, dh, lane);   // Q_h K_h^T
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (REL) {
              const float v = fmaxf(dp[t][r] * pr_prob(s[t][r], c, mrow[t][r], irow[t][r]), 0.f);
              acc[t][kb][r] = (h == h0) ? v : acc[t][kb][r] + v;
            } else {
              acc[t][kb][r] = dp[t][r];
            }
          }
      }
    }
    float (*tile)[PR_LD] = sT[wv];       // this wave's own tile: only wave-level ordering is needed
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[t][kb][r];
          if (REL) v = v / (float)heads;
          tile[16 * t + 4 * g + r][16 * kb + (lane & 15)] = v;
        }
    pr_store_tile(tile, obase, n, i0, valid_rows, j0, vec4, lane);
  }
}

// v_j = u_j + sum_i u_i A_ij for one layer; u = the previous step's vector, or (NULL) the start: e_0 (one row to read) or, with start_mean,
// 1 / n everywhere.  The last step writes the patch tokens j >= 1 to out [B, n - 1].  grid (ceil(n / 64), B), four waves over the rows.
__global__ __launch_bounds__(256) void relevance_gemv_kernel(const float* __restrict__ A, int n, const float* __restrict__ u, int start_mean,
                                                             float* __restrict__ v, int last) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, b = blockIdx.y, j = blockIdx.x * 64 + lane;
  const float* ub = u ? u + (long)b * n : nullptr;
  const float u0 = start_mean ? 1.0f / (float)n : 1.0f;
  const int nrows = (!u && !start_mean) ? 1 : n;
  float acc = 0.f;
  if (j < n) {
#pragma unroll 4
    for (int i = wid; i < nrows; i += 4) acc = __builtin_fmaf(ub ? ub[i] : u0, A[((long)b * n + i) * n + j], acc);
  }
  part[wid][lane] = acc;
  __syncthreads();
  if (wid == 0 && j < n) {
    const float uj = ub ? ub[j] : (start_mean || j == 0 ? u0 : 0.f);
    const float r = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) + uj;
    if (!last) v[(long)b * n + j] = r;
    else if (j >= 1) v[(long)b * (n - 1) + j - 1] = r;
  }
}

template <typename T, int KK, int RT>
void launch_grad16(const void* qkv, long ld, const void* dout, long ldo, int B, int n, int heads, int dh, float c, int form, float* out, hipStream_t s) {
  const int vec4 = (n % 4 == 0 && nv_aligned16(out)) ? 1 : 0;
  // key splits: enough workgroups to fill the chip (~4 per CU) while every wave keeps at least one 64-key chunk (as nv_attn_probs)
  const int tiles = (n + 16 * RT - 1) / (16 * RT), ys = form == NV_ATTN_GRAD_PER_HEAD ? B * heads : B;
  const int chunk_groups = ((n + 63) / 64 + PR_WAVES - 1) / PR_WAVES;
  const int ks = max(1, min(chunk_groups, (1024 + tiles * ys - 1) / (tiles * ys)));
  const dim3 grid(tiles, ys, ks);
#define GR16(F) hipLaunchKernelGGL((attn_grad16_kernel<T, KK, RT, F>), grid, dim3(64 * PR_WAVES), 0, s, (const r16*)qkv, ld, (const r16*)dout, ldo, n, heads, dh, c, out, vec4)
  if (form == NV_ATTN_GRAD_RELEVANCE) GR16(NV_ATTN_GRAD_RELEVANCE);
  else GR16(NV_ATTN_GRAD_PER_HEAD);
#undef GR16
}

template <typename T>
void dispatch_grad16(const void* qkv, long ld, const void* dout, long ldo, int B, int n, int heads, int dh, float c, int form, float* out, hipStream_t s) {
  switch ((dh + 31) / 32) {               // two row tiles per wave: each V (and K) fragment feeds two MFMAs
    case 1: launch_grad16<T, 1, 2>(qkv, ld, dout, ldo, B, n, heads, dh, c, form, out, s); break;
    case 2: launch_grad16<T, 2, 2>(qkv, ld, dout, ldo, B, n, heads, dh, c, form, out, s); break;
    case 3: launch_grad16<T, 3, 2>(qkv, ld, dout, ldo, B, n, heads, dh, c, form, out, s); break;
    default: launch_grad16<T, 4, 2>(qkv, ld, dout, ldo, B, n, heads, dh, c, form, out, s); break;
  }
}

}  // namespace

extern "C" int nv_attn_grad(const void* qkv, long ld_qkv, const void* dout, long ld_dout, int B, int n, int heads, int dim_head, float scale, int form,
                            float* out, void* stream) {
  NV_CHECK_ARG(qkv && dout && out && B > 0 && n > 0 && heads > 0 && scale > 0.f, "nv_attn_grad: bad shape / null pointer");
  NV_CHECK_ARG(form == NV_ATTN_GRAD_PER_HEAD || form == NV_ATTN_GRAD_RELEVANCE, "nv_attn_grad: form=%d out of range", form);
  NV_CHECK_ARG(dim_head >= 8 && dim_head <= 128 && dim_head % 8 == 0, "nv_attn_grad: dim_head must be a multiple of 8 up to 128, got %d", dim_head);
  NV_CHECK_ARG(ld_qkv >= 3L * heads * dim_head && ld_qkv % 8 == 0 && nv_aligned16(qkv),
               "nv_attn_grad: ld_qkv=%ld must cover q, k, v of every head and be a multiple of 8; qkv 16-byte aligned", ld_qkv);
  NV_CHECK_ARG(ld_dout >= (long)heads * dim_head && ld_dout % 8 == 0 && nv_aligned16(dout),
               "nv_attn_grad: ld_dout=%ld must cover every head and be a multiple of 8; dout 16-byte aligned", ld_dout);
  NV_CHECK_ARG(((uintptr_t)out & 3) == 0, "nv_attn_grad: out must be 4-byte aligned");
  NV_CHECK_ARG(form == NV_ATTN_GRAD_PER_HEAD || heads <= PR_MAXH, "nv_attn_grad: the relevance form supports up to %d heads", PR_MAXH);
  const float c = scale * PR_LOG2E;
  hipStream_t s = (hipStream_t)stream;
  NV_DISPATCH_OPERAND(T, dispatch_grad16<T>(qkv, ld_qkv, dout, ld_dout, B, n, heads, dim_head, c, form, out, s));
  NV_CHECK_LAUNCH("nv_attn_grad");
  return NV_OK;
}

extern "C" long nv_attn_relevance_workspace_bytes(int B, int n) { return (B > 0 && n > 0) ? 2L * B * n * (long)sizeof(float) : -1; }

extern "C" int nv_attn_relevance(const float* const* maps, int L, int B, int n, int start_mean, float* out, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(maps && out && workspace && L > 0 && B > 0 && n > 1, "nv_attn_relevance: bad shape / null pointer");
  NV_CHECK_ARG(ws_bytes >= nv_attn_relevance_workspace_bytes(B, n), "nv_attn_relevance: workspace too small (%ld < %ld)", ws_bytes,
               nv_attn_relevance_workspace_bytes(B, n));
  for (int l = 0; l < L; ++l) NV_CHECK_ARG(maps[l], "nv_attn_relevance: map of layer %d is NULL", l);
  hipStream_t s = (hipStream_t)stream;
  float* buf[2] = {(float*)workspace, (float*)workspace + (long)B * n};
  const float* u = nullptr;
  for (int l = L - 1, t = 0; l >= 0; --l, t ^= 1) {       // u (I + A_{L-1}) ... (I + A_0): the last layer first
    float* v = l == 0 ? out : buf[t];
    hipLaunchKernelGGL(relevance_gemv_kernel, dim3((n + 63) / 64, B), dim3(256), 0, s, maps[l], n, u, start_mean, v, l == 0 ? 1 : 0);
    u = v;
  }
  NV_CHECK_LAUNCH("nv_attn_relevance");
  return NV_OK;
}
