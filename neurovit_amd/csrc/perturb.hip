// Perturbation attribution on the device: the steps around the forward of deletion / insertion curves and of patch occlusion sensitivity
// (NeuroEncoder.perturbation_curves / occlusion_sensitivity).  The forward is the engine's; this file ranks the tokens of a map, writes
// the perturbed copies of a volume, and turns the logits of those copies into class scores, curve areas and occlusion maps.
//
//   nv_token_ranks       [B, N] maps -> [B, N] ranks (descending, ties to the lower token index): one workgroup per volume, keys in LDS
//   nv_mask_patches      x [B, S0, S1, S2] + labels [B, N] + jobs [J, 3] -> out [J, S0, S1, S2]: a pure select between x and a baseline,
//                        streamed with 16-byte stores; the volume's labels and the token index of every row / column sit in LDS
//   nv_mask_patches_rows the same kernel body over jobs [J, 4] = (b, row, lo, hi) whose label row is named by the job (labels [Rows, N]):
//                        many labellings of one volume in one call (NeuroEncoder.shapley_values)
//   nv_class_scores      logits [J, C] -> scores [J] (the logit, or the softmax probability) of the class of each job's source volume
//   nv_curve_auc         trapezoid area of [B, K] curves on the uniform grid k / (K - 1), summed in double
//   nv_occlusion_gather  maps[b, t] = ref[b] - scores[b, labels[b, t]]
//
// The only real bytes are the J * S0 * S1 * S2 * 4 of nv_mask_patches' output; everything else works on <= 4096 cells per volume.
#include "attr_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ ranks
constexpr int RK_THREADS = 256;
constexpr int RK_MAX_CELLS = 4096;       // 16 KB of keys in LDS (16^3 = ViT3D-large)

// One workgroup per volume: a counting pass over the keys (float_key; -0.0 and +0.0 share one key) in LDS.  Every lane of a wave reads
// the same four keys (one broadcast 16-byte LDS read) and compares them with its own token's key; the slots behind N hold key 0, which
// no finite value has and no comparison counts.
__global__ __launch_bounds__(RK_THREADS) void token_ranks_kernel(const float* __restrict__ maps, int N, int* __restrict__ ranks) {
  __shared__ u32x4 keys4[RK_MAX_CELLS / 4];
  unsigned* keys = reinterpret_cast<unsigned*>(keys4);
  const int tid = threadIdx.x;
  const long off = (long)blockIdx.x * N;
  const int N4 = (N + 3) >> 2;
  for (int i = tid; i < 4 * N4; i += RK_THREADS) {
    const float v = i < N ? maps[off + i] : 0.f;
    keys[i] = i < N ? float_key(v == 0.f ? 0.f : v) : 0u;      // -0.0 takes the key of +0.0
  }
  __syncthreads();
  for (int t = tid; t < N; t += RK_THREADS) {
    const unsigned mine = keys[t];
    int above = 0;
    for (int q = 0; q < N4; ++q) {
      const u32x4 k = keys4[q];
      const int j = 4 * q;
#pragma unroll
      for (int e = 0; e < 4; ++e) above += (k[e] > mine || (k[e] == mine && j + e < t)) ? 1 : 0;
    }
    ranks[off + t] = above;
  }
}

// ------------------------------------------------------------------------------------------------ masked copies
constexpr int MK_THREADS = 256;
constexpr int MK_MAX_CELLS = 4096;       // labels of one volume: 16 KB of LDS
constexpr int MK_MAX_GROUP = 16;         // jobs one workgroup serves from one read of its plane of x
int g_mask_group = 4;

// Grid (S0, ceil(J / group)).  A workgroup owns the S1 x S2 plane i0 of `group` consecutive jobs.  The jobs are taken in runs of equal
// source volume b (runs of one job when a volume is no multiple of four voxels, since the jobs' planes then differ in alignment): the labels
// of b are loaded into LDS once, and every 16-byte group of the plane reads x[b] (and the baseline), forms its four token indices and
// looks their labels up ONCE, then selects and stores for each job of the run.  The token of voxel
// (i0, i1, i2) is (i2 / p2) G0 G1 + (i0 / p0) G1 + i1 / p1: the row and column terms come from two LDS tables, so the stream divides once
// per group (flat plane offset -> row).  Groups of four follow the alignment of `out` (split_span);
// x and the baseline are read as 16-byte vectors when their plane has the same alignment as the output's (uniform per run), voxel by
// voxel otherwise.  Everything moves as 32-bit patterns: no arithmetic touches a voxel.
// JC = 3: a job is (b, lo, hi) and its label row is b (nv_mask_patches).  JC = 4: a job is (b, row, lo, hi) with its label row one of
// `rows` (nv_mask_patches_rows); a run then also shares the row, and a row outside [0, rows) skips the job as a volume outside [0, B) does.
template <int JC>
__global__ __launch_bounds__(MK_THREADS) void mask_patches_kernel(const unsigned* __restrict__ x, int B, int S0, int S1, int S2, int p0, int p1, int p2,
                                                                  const int* __restrict__ labels, const int* __restrict__ jobs, int J, int group,
                                                                  unsigned value, const unsigned* __restrict__ base, long base_stride,
                                                                  unsigned* __restrict__ out, int rows) {
  extern __shared__ int mk_smem[];
  const int G0 = S0 / p0, G1 = S1 / p1, G2 = S2 / p2, N = G0 * G1 * G2;
  int* lab = mk_smem;                                      // [N]
  int* row_tok = lab + N;                                  // [S1]: i1 / p1
  int* col_tok = row_tok + S1;                             // [S2]: (i2 / p2) G0 G1
  __shared__ int s_job[JC * MK_MAX_GROUP];
  const int tid = threadIdx.x, i0 = blockIdx.x;
  const int j_first = blockIdx.y * group, j_end = min(j_first + group, J);
  for (int i = tid; i < JC * (j_end - j_first); i += MK_THREADS) s_job[i] = jobs[(long)JC * j_first + i];
  for (int i = tid; i < S1; i += MK_THREADS) row_tok[i] = i / p1;
  for (int i = tid; i < S2; i += MK_THREADS) col_tok[i] = (i / p2) * G0 * G1;
  __syncthreads();
  const int plane_tok = (i0 / p0) * G1;
  const int P = S1 * S2;
  const long vol = (long)S0 * P;

  const bool same_alignment = (vol & 3) == 0;              // else consecutive jobs' planes differ in alignment: runs of one job
  const int n_jobs = j_end - j_first;
  int r0 = 0, loaded_row = -1;
  // (path_points_kernel of path_attr.hip walks the same runs over its pre-validated two-column jobs)
  while (r0 < n_jobs) {                                    // (every condition below is uniform over the workgroup)
    const int b = s_job[JC * r0];
    const int row = JC == 4 ? s_job[JC * r0 + 1] : b;
    int r1 = r0 + 1;
    while (same_alignment && r1 < n_jobs && s_job[JC * r1] == b && (JC == 3 || s_job[JC * r1 + 1] == row)) ++r1;
    if (b < 0 || b >= B || (JC == 4 && (row < 0 || row >= rows))) { r0 = r1; continue; }      // such a job reads nothing and writes nothing
    if (row != loaded_row) {
      __syncthreads();                                     // the previous run has finished with `lab`
      for (int i = tid; i < N; i += MK_THREADS) lab[i] = labels[(long)row * N + i];
      __syncthreads();
      loaded_row = row;
    }
    const unsigned* xp = x + (long)b * vol + (long)i0 * P;
    const unsigned* bp = base ? base + (long)b * base_stride + (long)i0 * P : nullptr;
    const long o_first = (long)(j_first + r0) * vol + (long)i0 * P;       // flat offset of the plane in `out`, first job of the run
    unsigned* o = out + o_first;                                          // (job r of the run: (r - r0) vol further, the same alignment)
    const Span s = split_span(o_first, P);                                // `out` is 16-byte aligned
    auto single = [&](int e) {                                            // one voxel, every job of the run
      const int y = e / S2, z = e - y * S2;
      const int l = lab[plane_tok + row_tok[y] + col_tok[z]];
      const unsigned xv = xp[e], bv = bp ? bp[e] : value;
      for (int r = r0; r < r1; ++r) o[(long)(r - r0) * vol + e] = (l >= s_job[JC * r + JC - 2] && l < s_job[JC * r + JC - 1]) ? bv : xv;
    };
    for (int e = tid; e < s.head; e += MK_THREADS) single(e);
    for (int e = s.tail + tid; e < P; e += MK_THREADS) single(e);
    const bool x_vec = is_aligned16(xp + s.head), b_vec = bp && is_aligned16(bp + s.head);
    for (int g = tid; g < s.groups; g += MK_THREADS) {
      const int e = s.head + 4 * g;
      int y = e / S2, z = e - y * S2;
      int rt = plane_tok + row_tok[y];
      const u32x4 xv = load4(xp + e, x_vec);
      const u32x4 bv = bp ? load4(bp + e, b_vec) : u32x4{value, value, value, value};
      int l[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        l[k] = lab[rt + col_tok[z]];
        if (++z == S2 && k < 3) { z = 0; ++y; rt = plane_tok + row_tok[y]; }     // (a group may straddle rows; y < S1 because e + k < P)
      }
      for (int r = r0; r < r1; ++r) {
        const int lo = s_job[JC * r + JC - 2], hi = s_job[JC * r + JC - 1];
        u32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (l[k] >= lo && l[k] < hi) ? bv[k] : xv[k];
        *reinterpret_cast<u32x4*>(o + (long)(r - r0) * vol + e) = v;
      }
    }
    r0 = r1;
  }
}

// ------------------------------------------------------------------------------------------------ scores, areas, occlusion maps
constexpr int CS_THREADS = 256;
constexpr int CS_WAVES = CS_THREADS / 64;

// One wave per job.  kind 1: the class logit as it is.  kind 0: exp(l_c - max) / sum_i exp(l_i - max) in fp32 (wave_softmax_stats).
// A job whose source volume is outside [0, B) writes nothing; a class outside [0, C) gives NaN.
__global__ __launch_bounds__(CS_THREADS) void class_scores_kernel(const float* __restrict__ logits, int J, int C, const int* __restrict__ jobs,
                                                                  const long* __restrict__ cls, int B, int kind, float* __restrict__ scores) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * CS_WAVES + (threadIdx.x >> 6);
  if (j >= J) return;
  const int b = jobs[3L * j];
  if (b < 0 || b >= B) return;
  const long c = cls[b];
  const float* row = logits + (long)j * C;
  if (c < 0 || c >= C) {
    if (lane == 0) scores[j] = __uint_as_float(0x7fc00000u);
    return;
  }
  if (kind == 1) {
    if (lane == 0) scores[j] = row[c];
    return;
  }
  float mx, sum;
  wave_softmax_stats(row, C, lane, mx, sum);
  if (lane == 0) scores[j] = expf(row[c] - mx) / sum;
}

// One thread per curve: (sum_k s_k - (s_0 + s_{K-1}) / 2) / (K - 1), summed in double in index order, stored as fp32.
__global__ void curve_auc_kernel(const float* __restrict__ scores, int B, int K, long ld, float* __restrict__ auc) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* s = scores + (long)b * ld;
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += (double)s[k];
  auc[b] = (float)((sum - ((double)s[0] + (double)s[K - 1]) / 2.0) / (double)(K - 1));
}

// maps[b, t] = ref[b] - scores[b, labels[b, t]]  (scores [B, NB]); a label outside [0, NB) gives NaN.
__global__ void occlusion_gather_kernel(const float* __restrict__ ref, const float* __restrict__ scores, const int* __restrict__ labels, int B, int N,
                                        int NB, float* __restrict__ maps) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * N) return;
  const int b = (int)(i / N), l = labels[i];
  maps[i] = (l >= 0 && l < NB) ? ref[b] - scores[(long)b * NB + l] : __uint_as_float(0x7fc00000u);
}
}  // namespace

extern "C" int nv_token_ranks(const float* maps, int B, int N, int* ranks, void* stream) {
  NV_CHECK_ARG(maps && ranks && B > 0 && N > 0, "nv_token_ranks: bad arguments (null pointer, or B / N not positive)");
  NV_CHECK_ARG(N <= RK_MAX_CELLS, "nv_token_ranks: %d tokens, the kernel takes at most %d (16^3)", N, RK_MAX_CELLS);
  NV_CHECK_ARG(nv_aligned(maps, 4) && nv_aligned(ranks, 4), "nv_token_ranks: maps / ranks 4-byte aligned");
  hipLaunchKernelGGL(token_ranks_kernel, dim3(B), dim3(RK_THREADS), 0, (hipStream_t)stream, maps, N, ranks);
  NV_CHECK_LAUNCH("nv_token_ranks");
  return NV_OK;
}

extern "C" int nv_mask_patches_set_group(int group) {
  if (group < 1 || group > MK_MAX_GROUP) {
    nv_set_error("nv_mask_patches_set_group: group %d outside [1, %d]", group, MK_MAX_GROUP);
    return NV_ERR_ARG;
  }
  g_mask_group = group;
  return NV_OK;
}

// the checks and the launch of nv_mask_patches (JC = 3, rows unused) and nv_mask_patches_rows (JC = 4)
template <int JC>
static int mask_patches_launch(const char* name, const float* x, int B, const int* size3, const int* patch3, const int* labels, int rows, const int* jobs,
                               int J, float value, const float* base, long base_stride, float* out, void* stream) {
  NV_CHECK_ARG(x && size3 && patch3 && labels && jobs && out && B > 0 && J > 0 && rows > 0, "%s: bad arguments (null pointer, or B / J%s not positive)", name,
               JC == 4 ? " / Rows" : "");
  const int S0 = size3[0], S1 = size3[1], S2 = size3[2], p0 = patch3[0], p1 = patch3[1], p2 = patch3[2];
  NV_CHECK_ARG(S0 > 0 && S1 > 0 && S2 > 0 && p0 > 0 && p1 > 0 && p2 > 0, "%s: volume and patch extents must be positive", name);
  NV_CHECK_ARG(S0 % p0 == 0 && S1 % p1 == 0 && S2 % p2 == 0, "%s: volume %d x %d x %d is not a whole number of %d x %d x %d patches", name, S0, S1, S2,
               p0, p1, p2);
  const long N = (long)(S0 / p0) * (S1 / p1) * (S2 / p2);
  NV_CHECK_ARG(N <= MK_MAX_CELLS, "%s: %ld patches, the kernel takes at most %d (16^3)", name, N, MK_MAX_CELLS);
  const long lds = (N + S1 + S2) * 4;
  NV_CHECK_ARG(lds <= 65536 - 256 && (long)S1 * S2 < (1L << 31), "%s: extents %d x %d x %d beyond the kernel's tables (patches + S1 + S2 <= 16320)", name, S0,
               S1, S2);
  const int group = g_mask_group;
  const long job_groups = ((long)J + group - 1) / group;
  NV_CHECK_ARG(job_groups <= 65535, "%s: %d jobs, at most %d in one call", name, J, 65535 * group);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned(x, 4) && nv_aligned(base, 4) && nv_aligned(labels, 4) && nv_aligned(jobs, 4),
               "%s: out 16-byte aligned, every other buffer 4-byte aligned", name);
  NV_CHECK_ARG(base_stride == 0 || base_stride >= (long)S0 * S1 * S2, "%s: baseline stride %ld is neither 0 nor at least one volume", name, base_stride);
  union { float f; unsigned u; } vbits;
  vbits.f = value;
  hipLaunchKernelGGL(mask_patches_kernel<JC>, dim3(S0, (unsigned)job_groups), dim3(MK_THREADS), (size_t)lds, (hipStream_t)stream, (const unsigned*)x, B, S0, S1,
                     S2, p0, p1, p2, labels, jobs, J, group, vbits.u, (const unsigned*)base, base_stride, (unsigned*)out, rows);
  NV_CHECK_LAUNCH(name);
  return NV_OK;
}

extern "C" int nv_mask_patches(const float* x, int B, const int* size3, const int* patch3, const int* labels, const int* jobs, int J, float value,
                               const float* base, long base_stride, float* out, void* stream) {
  return mask_patches_launch<3>("nv_mask_patches", x, B, size3, patch3, labels, B, jobs, J, value, base, base_stride, out, stream);
}

extern "C" int nv_mask_patches_rows(const float* x, int B, const int* size3, const int* patch3, const int* labels, int Rows, const int* jobs, int J, float value,
                                    const float* base, long base_stride, float* out, void* stream) {
  return mask_patches_launch<4>("nv_mask_patches_rows", x, B, size3, patch3, labels, Rows, jobs, J, value, base, base_stride, out, stream);
}

extern "C" int nv_class_scores(const float* logits, int J, int C, const int* jobs, const long* cls, int B, int kind, float* scores, void* stream) {
  NV_CHECK_ARG(logits && jobs && cls && scores && J > 0 && C > 0 && B > 0, "nv_class_scores: bad arguments (null pointer, or J / C / B not positive)");
  NV_CHECK_ARG(kind == NV_SCORE_PROB || kind == NV_SCORE_LOGIT, "nv_class_scores: kind %d is neither NV_SCORE_PROB nor NV_SCORE_LOGIT", kind);
  NV_CHECK_ARG(nv_aligned(logits, 4) && nv_aligned(jobs, 4) && nv_aligned(cls, 8) && nv_aligned(scores, 4),
               "nv_class_scores: element-aligned buffers");
  hipLaunchKernelGGL(class_scores_kernel, dim3((J + CS_WAVES - 1) / CS_WAVES), dim3(CS_THREADS), 0, (hipStream_t)stream, logits, J, C, jobs, cls, B, kind, scores);
  NV_CHECK_LAUNCH("nv_class_scores");
  return NV_OK;
}

extern "C" int nv_curve_auc(const float* scores, int B, int K, long ld, float* auc, void* stream) {
  NV_CHECK_ARG(scores && auc && B > 0 && K >= 2 && ld >= K, "nv_curve_auc: bad arguments (null pointer, B < 1, K < 2 or ld < K)");
  NV_CHECK_ARG(nv_aligned(scores, 4) && nv_aligned(auc, 4), "nv_curve_auc: element-aligned buffers");
  hipLaunchKernelGGL(curve_auc_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, scores, B, K, ld, auc);
  NV_CHECK_LAUNCH("nv_curve_auc");
  return NV_OK;
}

extern "C" int nv_occlusion_gather(const float* ref, const float* scores, const int* labels, int B, int N, int NB, float* maps, void* stream) {
  NV_CHECK_ARG(ref && scores && labels && maps && B > 0 && N > 0 && NB > 0, "nv_occlusion_gather: bad arguments (null pointer, or B / N / NB not positive)");
  NV_CHECK_ARG(nv_aligned(ref, 4) && nv_aligned(scores, 4) && nv_aligned(labels, 4) && nv_aligned(maps, 4),
               "nv_occlusion_gather: element-aligned buffers");
  const long total = (long)B * N;
  NV_CHECK_ARG((total + 255) / 256 < (1L << 31), "nv_occlusion_gather: B N too large");
  hipLaunchKernelGGL(occlusion_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ref, scores, labels, B, N, NB, maps);
  NV_CHECK_LAUNCH("nv_occlusion_gather");
  return NV_OK;
}
