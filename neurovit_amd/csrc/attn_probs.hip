// Attention probabilities and attention rollout (explainability; vit_3d.py:54 `self.attend = nn.Softmax(dim=-1)`).
//
// The flash-style attention kernels never materialise P = softmax(scale q k^T).  These kernels recompute it from a layer's qkv
// buffer, behind the attention launch that read the same buffer, and write it in the layout of the reference's `attend` output
// ([B, heads, n, n] after 'b n (h d) -> b h n d'), or fused over the heads (mean / max / min), or only its cls row.
//
//   attn_probs16_kernel   16-bit qkv (operand format): S = Q K^T on v_mfma_f32_16x16x32, fp32 accumulation.  A workgroup of four
//                         waves per 16 * RT query rows of one (volume, head) - or of one volume and every head (fused forms) - and
//                         per key split.  Pass 1 sweeps the keys once for each row's max and sum (online, merged across the 16 lanes
//                         of a row group, then across the four waves); pass 2 recomputes S 64 keys at a time, forms
//                         p = exp2(s c - m) / l, and - the kernel is bound by its fp32 output - transposes the column-major C
//                         fragments through LDS so that every store instruction writes whole 64-key runs of a row (256 contiguous
//                         bytes; float4 per lane when n % 4 == 0 keeps the rows 16-byte aligned).
//   attn_probs32_kernel   fp32 qkv (precision("fp32") path): one wave per query row, lanes over the keys, exact max then sum, fp32
//                         FMA chains.  For accuracy, not speed; the fused forms combine the heads in place in the output row.
//   rollout kernels       u <- u A^ with A^ = (A + I) / (rowsum(A) + 1), a batched GEMV per layer (memory-bound): one launch forms
//                         w_i = u_i / (rowsum_i + 1), the next v_j = sum_i w_i A_ij + w_j.
//
// A row's probabilities come out bit-identical in every form (same MFMA order, same statistics): max / min fusion equals the
// reduction of the per-head export exactly, and the cls form equals row 0 of the all-rows form.  The fragment loads, the score tile, the
// statistics sweep, the exp2 expression and the transposed store live in attn_probs.h: attn_grad.hip forms the same probabilities from them.
#include "attn_probs.h"

namespace {

__device__ __forceinline__ float pr_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

template <int FUSE>
__device__ __forceinline__ float pr_fuse(float acc, float p, bool first) {
  if (first) return p;
  if constexpr (FUSE == NV_ATTN_FUSE_MAX) return fmaxf(acc, p);
  else if constexpr (FUSE == NV_ATTN_FUSE_MIN) return fminf(acc, p);
  else return acc + p;                    // mean: the division by heads follows the last head
}

// grid (ceil(rows / (16 RT)), B * heads [per head] or B [fused], KS), four waves.  The workgroup's waves share its 16 RT query rows and
// split the keys: in pass 1 wave w sweeps the 16-key blocks w, w + 4, ... and the four partial statistics are merged through LDS in wave
// order (every workgroup, every form: the same bits); in pass 2 wave w of key split z writes the 64-key chunks 4 z + w, + 4 KS, ...
// out: [B, heads, rows, n] or [B, rows, n] fp32, rows = n or 1.
template <typename T, int KK, int RT, int FUSE>
__global__ __launch_bounds__(64 * PR_WAVES) void attn_probs16_kernel(const r16* __restrict__ qkv, long ld, int n, int heads, int dh, float c,
                                                                     int rows, float* __restrict__ out, int vec4) {
  __shared__ __attribute__((aligned(16))) float sT[PR_WAVES][16 * RT][PR_LD];
  __shared__ float sPart[PR_WAVES][16 * RT][2];
  __shared__ float sSt[FUSE == NV_ATTN_PER_HEAD ? 1 : PR_MAXH][16 * RT][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, i0 = blockIdx.x * 16 * RT;
  const int inner = heads * dh;
  int b, h0, h1;
  if (FUSE == NV_ATTN_PER_HEAD) { b = blockIdx.y / heads; h0 = blockIdx.y - b * heads; h1 = h0 + 1; }
  else { b = blockIdx.y; h0 = 0; h1 = heads; }
  const r16* base = qkv + (long)b * n * ld;
  float* obase = out + (long)blockIdx.y * rows * n;
  r16x8 qf[RT][KK];
  f32x4 s[RT];
  float mrow[RT][4], irow[RT][4];          // per-head form: the statistics stay in registers

  // ---- pass 1: row max and sum of every head this workgroup serves
  for (int h = h0; h < h1; ++h) {
    pr_load_q<KK, RT>(qf, base, ld, i0, rows, h * dh, dh, lane);
    pr_row_stats<T, KK, RT>(mrow, irow, qf, base, ld, n, inner + h * dh, dh, c, sPart, lane, wv);
    if (FUSE != NV_ATTN_PER_HEAD && wv == 0 && (lane & 15) == 0) {
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) { sSt[h][16 * t + 4 * g + r][0] = mrow[t][r]; sSt[h][16 * t + 4 * g + r][1] = irow[t][r]; }
    }
    __syncthreads();                     // sPart is rewritten by the next head
  }

  // ---- pass 2: 64 keys at a time: probabilities (fused over the heads), transposed through LDS, stored as row runs
  const int valid_rows = min(16 * RT, rows - i0);
  for (int j0 = 64 * (PR_WAVES * blockIdx.z + wv); j0 < n; j0 += 64 * PR_WAVES * gridDim.z) {
    float acc[RT][4][4];
    for (int h = h0; h < h1; ++h) {
      if (FUSE != NV_ATTN_PER_HEAD) {
        pr_load_q<KK, RT>(qf, base, ld, i0, rows, h * dh, dh, lane);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) { mrow[t][r] = sSt[h][16 * t + 4 * g + r][0]; irow[t][r] = sSt[h][16 * t + 4 * g + r][1]; }
      }
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (j0 + 16 * kb >= n) break;                                   // wave-uniform
        pr_scores<T, KK, RT>(s, qf, base, ld, n, j0 + 16 * kb, inner + h * dh, dh, lane);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float p = pr_prob(s[t][r], c, mrow[t][r], irow[t][r]);
            acc[t][kb][r] = pr_fuse<FUSE>(acc[t][kb][r], p, h == h0);
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
          if (FUSE == NV_ATTN_FUSE_MEAN) v = v / (float)heads;
          tile[16 * t + 4 * g + r][16 * kb + (lane & 15)] = v;
        }
    pr_store_tile(tile, obase, n, i0, valid_rows, j0, vec4, lane);
  }
}

// fp32 qkv: grid (ceil(rows / 4), B * heads [per head] or B [fused]), four waves, one query row each
template <int FUSE>
__global__ __launch_bounds__(256) void attn_probs32_kernel(const float* __restrict__ qkv, long ld, int n, int heads, int dh, float c, int rows,
                                                           float* __restrict__ out) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= rows) return;
  const int inner = heads * dh;
  int b, h0, h1;
  if (FUSE == NV_ATTN_PER_HEAD) { b = blockIdx.y / heads; h0 = blockIdx.y - b * heads; h1 = h0 + 1; }
  else { b = blockIdx.y; h0 = 0; h1 = heads; }
  const float* base = qkv + (long)b * n * ld;
  float* orow = out + ((long)blockIdx.y * rows + i) * n;
  for (int h = h0; h < h1; ++h) {
    const float* q = base + (long)i * ld + h * dh;
    auto score = [&](int j) -> float {
      const float* k = base + (long)j * ld + inner + h * dh;
      float acc = 0.f;
      for (int e = 0; e < dh; e += 4) {
        const float4 a = *reinterpret_cast<const float4*>(q + e), x = *reinterpret_cast<const float4*>(k + e);
        acc = __builtin_fmaf(a.x, x.x, acc); acc = __builtin_fmaf(a.y, x.y, acc);
        acc = __builtin_fmaf(a.z, x.z, acc); acc = __builtin_fmaf(a.w, x.w, acc);
      }
      return acc * c;
    };
    float m = -INFINITY;
    for (int j = lane; j < n; j += 64) m = fmaxf(m, score(j));
    m = pr_wave_max(m);
    float l = 0.f;
    for (int j = lane; j < n; j += 64) l += __builtin_amdgcn_exp2f(score(j) - m);
    const float il = 1.0f / wave_sum(l);
    for (int j = lane; j < n; j += 64) {
      const float p = __builtin_amdgcn_exp2f(score(j) - m) * il;
      float v = pr_fuse<FUSE>(h == h0 ? 0.f : orow[j], p, h == h0);       // the lane re-reads only what it wrote itself
      if (FUSE == NV_ATTN_FUSE_MEAN && h == h1 - 1) v = v / (float)heads;
      orow[j] = v;
    }
  }
}

// rollout step, part 1: w[b, i] = u_i / (rowsum_i(A_b) + 1); u = the previous step's vector, or the start (cls row / mean of the rows)
__global__ __launch_bounds__(256) void rollout_scale_kernel(const float* __restrict__ A, int n, const float* __restrict__ u, int start_mean,
                                                            float* __restrict__ w) {
  const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (i >= n) return;
  const float* row = A + ((long)b * n + i) * n;
  float s = 0.f;
  for (int j = lane; j < n; j += 64) s += row[j];
  s = wave_sum(s);
  if (lane == 0) {
    const float ui = u ? u[(long)b * n + i] : (start_mean ? 1.0f / (float)n : (i == 0 ? 1.f : 0.f));
    w[(long)b * n + i] = ui / (s + 1.0f);
  }
}

// rollout step, part 2: v_j = sum_i w_i A_ij + w_j; the last step writes the patch tokens j >= 1 to out [B, n - 1]
__global__ __launch_bounds__(256) void rollout_gemv_kernel(const float* __restrict__ A, int n, const float* __restrict__ w, float* __restrict__ v,
                                                           int last) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, b = blockIdx.y, j = blockIdx.x * 64 + lane;
  const float* wb = w + (long)b * n;
  float acc = 0.f;
  if (j < n)
    for (int i = wid; i < n; i += 4) acc = __builtin_fmaf(wb[i], A[((long)b * n + i) * n + j], acc);
  part[wid][lane] = acc;
  __syncthreads();
  if (wid == 0 && j < n) {
    const float r = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) + wb[j];
    if (!last) v[(long)b * n + j] = r;
    else if (j >= 1) v[(long)b * (n - 1) + j - 1] = r;
  }
}

template <typename T, int KK, int RT>
void launch_probs16(const void* qkv, long ld, int B, int n, int heads, int dh, float c, int fusion, int rows, float* out, hipStream_t s) {
  const int vec4 = (n % 4 == 0 && nv_aligned16(out)) ? 1 : 0;
  // key splits: enough workgroups to fill the chip (~4 per CU) while every wave keeps at least one 64-key chunk of pass 2
  const int tiles = (rows + 16 * RT - 1) / (16 * RT), ys = fusion == NV_ATTN_PER_HEAD ? B * heads : B;
  const int chunk_groups = ((n + 63) / 64 + PR_WAVES - 1) / PR_WAVES;
  const int ks = max(1, min(chunk_groups, (1024 + tiles * ys - 1) / (tiles * ys)));
  const dim3 grid(tiles, ys, ks);
#define PR16(F) hipLaunchKernelGGL((attn_probs16_kernel<T, KK, RT, F>), grid, dim3(64 * PR_WAVES), 0, s, (const r16*)qkv, ld, n, heads, dh, c, rows, out, vec4)
  switch (fusion) {
    case NV_ATTN_FUSE_MEAN: PR16(NV_ATTN_FUSE_MEAN); break;
    case NV_ATTN_FUSE_MAX: PR16(NV_ATTN_FUSE_MAX); break;
    case NV_ATTN_FUSE_MIN: PR16(NV_ATTN_FUSE_MIN); break;
    default: PR16(NV_ATTN_PER_HEAD); break;
  }
#undef PR16
}

template <typename T, int RT>
void dispatch_probs16(const void* qkv, long ld, int B, int n, int heads, int dh, float c, int fusion, int rows, float* out, hipStream_t s) {
  switch ((dh + 31) / 32) {
    case 1: launch_probs16<T, 1, RT>(qkv, ld, B, n, heads, dh, c, fusion, rows, out, s); break;
    case 2: launch_probs16<T, 2, RT>(qkv, ld, B, n, heads, dh, c, fusion, rows, out, s); break;
    case 3: launch_probs16<T, 3, RT>(qkv, ld, B, n, heads, dh, c, fusion, rows, out, s); break;
    default: launch_probs16<T, 4, RT>(qkv, ld, B, n, heads, dh, c, fusion, rows, out, s); break;
  }
}

}  // namespace

extern "C" int nv_attn_probs(int qkv_f32, const void* qkv, long ld_qkv, int B, int n, int heads, int dim_head, float scale, int fusion, int rows,
                             float* out, void* stream) {
  NV_CHECK_ARG(qkv && out && B > 0 && n > 0 && heads > 0 && scale > 0.f, "nv_attn_probs: bad shape / null pointer");
  NV_CHECK_ARG(fusion >= NV_ATTN_PER_HEAD && fusion <= NV_ATTN_FUSE_MIN && (rows == NV_ATTN_ROWS_ALL || rows == NV_ATTN_ROWS_CLS),
               "nv_attn_probs: fusion=%d / rows=%d out of range", fusion, rows);
  NV_CHECK_ARG(ld_qkv >= 3L * heads * dim_head && nv_aligned16(qkv), "nv_attn_probs: ld_qkv=%ld must cover q, k, v of every head; qkv 16-byte aligned", ld_qkv);
  NV_CHECK_ARG(((uintptr_t)out & 3) == 0, "nv_attn_probs: out must be 4-byte aligned");
  const int nrows = rows == NV_ATTN_ROWS_CLS ? 1 : n;
  const float c = scale * PR_LOG2E;
  hipStream_t s = (hipStream_t)stream;
  if (qkv_f32) {
    NV_CHECK_ARG(dim_head >= 4 && dim_head <= 128 && dim_head % 4 == 0 && ld_qkv % 4 == 0,
                 "nv_attn_probs: fp32 qkv needs dim_head a multiple of 4 up to 128 and ld_qkv %% 4 == 0");
    const dim3 grid((nrows + 3) / 4, fusion == NV_ATTN_PER_HEAD ? B * heads : B);
#define PR32(F) hipLaunchKernelGGL((attn_probs32_kernel<F>), grid, dim3(256), 0, s, (const float*)qkv, ld_qkv, n, heads, dim_head, c, nrows, out)
    switch (fusion) {
      case NV_ATTN_FUSE_MEAN: PR32(NV_ATTN_FUSE_MEAN); break;
      case NV_ATTN_FUSE_MAX: PR32(NV_ATTN_FUSE_MAX); break;
      case NV_ATTN_FUSE_MIN: PR32(NV_ATTN_FUSE_MIN); break;
      default: PR32(NV_ATTN_PER_HEAD); break;
    }
#undef PR32
    NV_CHECK_LAUNCH("nv_attn_probs/f32");
    return NV_OK;
  }
  NV_CHECK_ARG(dim_head >= 8 && dim_head <= 128 && dim_head % 8 == 0 && ld_qkv % 8 == 0,
               "nv_attn_probs: 16-bit qkv needs dim_head a multiple of 8 up to 128 and ld_qkv %% 8 == 0");
  NV_CHECK_ARG(fusion == NV_ATTN_PER_HEAD || heads <= PR_MAXH, "nv_attn_probs: head fusion supports up to %d heads", PR_MAXH);
  // two row tiles per wave (each key fragment feeds two MFMAs) for the all-rows forms; the cls form has one row
  if (nrows == 1) NV_DISPATCH_OPERAND(T, dispatch_probs16<T, 1>(qkv, ld_qkv, B, n, heads, dim_head, c, fusion, nrows, out, s));
  else NV_DISPATCH_OPERAND(T, dispatch_probs16<T, 2>(qkv, ld_qkv, B, n, heads, dim_head, c, fusion, nrows, out, s));
  NV_CHECK_LAUNCH("nv_attn_probs");
  return NV_OK;
}

extern "C" long nv_attn_rollout_workspace_bytes(int B, int n) { return (B > 0 && n > 0) ? 2L * B * n * (long)sizeof(float) : -1; }

extern "C" int nv_attn_rollout(const float* const* maps, int L, int B, int n, int start_mean, float* out, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(maps && out && workspace && L > 0 && B > 0 && n > 1, "nv_attn_rollout: bad shape / null pointer");
  NV_CHECK_ARG(ws_bytes >= nv_attn_rollout_workspace_bytes(B, n), "nv_attn_rollout: workspace too small (%ld < %ld)", ws_bytes,
               nv_attn_rollout_workspace_bytes(B, n));
  for (int l = 0; l < L; ++l) NV_CHECK_ARG(maps[l], "nv_attn_rollout: map of layer %d is NULL", l);
  hipStream_t s = (hipStream_t)stream;
  float* w = (float*)workspace;
  float* u = w + (long)B * n;
  for (int l = L - 1; l >= 0; --l) {             // u A^_{L-1} ... A^_0: the last layer first
    hipLaunchKernelGGL(rollout_scale_kernel, dim3((n + 3) / 4, B), dim3(256), 0, s, maps[l], n, l == L - 1 ? (const float*)nullptr : u, start_mean, w);
    hipLaunchKernelGGL(rollout_gemv_kernel, dim3((n + 63) / 64, B), dim3(256), 0, s, maps[l], n, (const float*)w, l == 0 ? out : u, l == 0 ? 1 : 0);
  }
  NV_CHECK_LAUNCH("nv_attn_rollout");
  return NV_OK;
}
