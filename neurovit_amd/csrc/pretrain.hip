// Masked-volume pretraining on the device (SimMIM / MAE on 3D volumes): the steps around the encoder's forward and backward.
//
//   nv_mim_labels        (seed, rank, step) -> labels int32 [B, N]: a fresh random mask per sample and step, drawn per mask unit (a cube of
//                        u^3 patches) and ranked in LDS; label < m means masked, so nv_mask_patches with the job (b, 0, m) writes the
//                        masked batch.  Nothing is read back, the host draws nothing.
//   nv_recon_loss        pred fp32 [B n, ldp] + the ORIGINAL volume + labels -> dpred (operand format) [B n, ldd] + per-row loss partials
//                        (double) + loss fp32 [1].  One workgroup per token row; the target patch is gathered once into LDS and serves the
//                        statistics pass (norm_pix) and the loss pass.  No atomics: every output cell is owned by one thread.
//   nv_token_grad_seed   dtokens fp32 [M, d] -> the three things the encoder's backward expects in front of its last layer: g = dtokens,
//                        g16 = cvt(dtokens * mask), and per-workgroup partial column sums of dtokens * mask (the FC2 bias gradient).
#include "attr_common.h"

#pragma clang fp contract(off)

namespace {
// ------------------------------------------------------------------------------------------------ labels
constexpr int ML_THREADS = 1024;
constexpr int ML_MAX_CELLS = 4096;       // patches (and so units) of one volume: 16 KB of keys in LDS
constexpr uint64_t MIM_DOMAIN = 0x4D494Dull;     // ABI: the header states the draw rule
constexpr unsigned MIM_STRIDE = 4096;

struct MimGeom { int G0, G1, G2, u, U0, U1, U2; };

// One workgroup per sample.  The key of unit q is the top 24 bits of its draw as an fp32 in [0, 1) (exact); the units are ranked by
// nv_token_ranks' rule (descending, ties to the lower index) with its counting pass over the keys in LDS (every lane of a wave reads the
// same four keys per 16-byte read; the slots behind U hold key 0, which no key of a value >= 0 has and no comparison counts), then every
// patch takes rank(unit) u^3 + its index inside the unit.  Patch and unit indices both follow nv_mask_patches' token rule (axis 2 slowest,
// then 0, then 1).
__global__ __launch_bounds__(ML_THREADS) void mim_labels_kernel(uint64_t seed, uint64_t rank, uint64_t step, MimGeom g, int* __restrict__ labels) {
  __shared__ u32x4 keys4[ML_MAX_CELLS / 4];
  __shared__ int urank[ML_MAX_CELLS];
  unsigned* keys = reinterpret_cast<unsigned*>(keys4);
  const int tid = threadIdx.x, b = blockIdx.x;
  const int U = g.U0 * g.U1 * g.U2, N = g.G0 * g.G1 * g.G2, u3 = g.u * g.u * g.u;
  const int U4 = (U + 3) >> 2;
  const uint64_t seed_m = nv_hash64(nv_hash64(seed, rank), MIM_DOMAIN);
  const uint64_t counter = ((step << 32) + (uint64_t)b) * MIM_STRIDE;
  for (int q = tid; q < 4 * U4; q += ML_THREADS) {
    const float key = (float)(unsigned)(nv_hash64(seed_m, counter + (uint64_t)q) >> 40) * 0x1p-24f;
    keys[q] = q < U ? float_key(key) : 0u;
  }
  __syncthreads();
  for (int q = tid; q < U; q += ML_THREADS) {
    const unsigned mine = keys[q];
    int above = 0;
    for (int j4 = 0; j4 < U4; ++j4) {
      const u32x4 k = keys4[j4];
#pragma unroll
      for (int e = 0; e < 4; ++e) above += (k[e] > mine || (k[e] == mine && 4 * j4 + e < q)) ? 1 : 0;
    }
    urank[q] = above;
  }
  __syncthreads();
  for (int t = tid; t < N; t += ML_THREADS) {
    const int g2 = t / (g.G0 * g.G1), rem = t - g2 * g.G0 * g.G1, g0 = rem / g.G1, g1 = rem - g0 * g.G1;
    const int q = ((g2 / g.u) * g.U0 + g0 / g.u) * g.U1 + g1 / g.u;
    const int inside = ((g2 % g.u) * g.u + g0 % g.u) * g.u + g1 % g.u;
    labels[(long)b * N + t] = urank[q] * u3 + inside;
  }
}

// ------------------------------------------------------------------------------------------------ reconstruction loss
constexpr int RL_THREADS = 256;
constexpr int RL_MAX_P = 4096;           // voxels of one patch (16^3): 16 KB of LDS
constexpr int RL_GROUPS = RL_MAX_P / 8 / RL_THREADS;      // groups of eight columns a thread serves

struct ReconGeom {
  int B, S0, S1, S2, p0, p1, p2, G0, G1, N, n, P, P8;
};

// double -> operand format with ONE rounding: the fp32 in between is rounded to odd (the inexact bit is kept in its last place), so
// the round-to-nearest-even that follows sees on which side of a 16-bit midpoint the double lay
template <typename T>
__device__ __forceinline__ r16 cvt1_once(double v) {
  float f = (float)v;
  if ((double)f != v && !(v != v)) {
    unsigned u = __float_as_uint(f);
    if (fabs((double)f) > fabs(v)) --u;       // towards zero (f is finite and non-zero here: a double of fp32 range)
    f = __uint_as_float(u | 1u);
  }
  return cvt1<T>(f);
}

// the sum of `v` over the workgroup's 256 threads, in every thread: the wave butterflies, then the four waves in order
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_sum(v);
  if (lane == 0) red[wid] = v;
  __syncthreads();
  const double s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// One workgroup per token row r = b n + i (i = 0: the cls row).  A row that is not masked writes zeros and a zero partial and reads
// neither pred nor the volume.  A masked row gathers its patch - p0 p1 runs of p2 contiguous floats, element order (a0 p1 + a1) p2 + a2
// = 'p1 p2 pf' of the engine's patchify - into LDS (VEC: 16-byte loads, every run starting on a 16-byte boundary; else dwords), forms
// mean and unbiased variance in double from there (norm_pix), then walks pred in groups of eight columns: two 16-byte loads, the loss
// terms in double, one 16-byte store of dpred.  kind 0: L1, 1: L2.  inv_count = 1 / (B m P); gscale = loss_scale (x 2 for L2) / (B m P).
template <typename T, bool VEC>
__global__ __launch_bounds__(RL_THREADS) void recon_loss_kernel(const float* __restrict__ pred, long ldp, const float* __restrict__ x, ReconGeom g,
                                                                const int* __restrict__ labels, int m, int kind, int norm_pix, double inv_count,
                                                                double gscale, r16* __restrict__ dpred, long ldd, double* __restrict__ partials) {
  __shared__ f32x4 tgt4[RL_MAX_P / 4];
  __shared__ double red[4];
  float* tgt = reinterpret_cast<float*>(tgt4);
  const int tid = threadIdx.x;
  const long r = blockIdx.x;
  const int b = (int)(r / g.n), i = (int)(r - (long)b * g.n);
  r16* drow = dpred + r * ldd;
  const int groups_row = (int)(ldd >> 3);
  const r16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const bool masked = i > 0 && labels[(long)b * g.N + (i - 1)] < m;        // workgroup-uniform
  if (!masked) {
    for (int q = tid; q < groups_row; q += RL_THREADS) *reinterpret_cast<r16x8*>(drow + 8 * q) = zero8;
    if (tid == 0) partials[r] = 0.0;
    return;
  }
  // pred of this thread's (at most two) column groups: asked for first, so that its latency runs under the gather and the statistics
  const float* prow = pred + r * ldp;
  f32x4 pa[RL_GROUPS], pb[RL_GROUPS];
#pragma unroll
  for (int j = 0; j < RL_GROUPS; ++j) {
    const int c = 8 * (tid + j * RL_THREADS);
    if (c < g.P8) { pa[j] = *reinterpret_cast<const f32x4*>(prow + c); pb[j] = *reinterpret_cast<const f32x4*>(prow + c + 4); }
  }
  const int t = i - 1;
  const int g2 = t / (g.G0 * g.G1), rem = t - g2 * g.G0 * g.G1, g0 = rem / g.G1, g1 = rem - g0 * g.G1;
  const float* base = x + (((long)b * g.S0 + (long)g0 * g.p0) * g.S1 + (long)g1 * g.p1) * g.S2 + (long)g2 * g.p2;
  if constexpr (VEC) {
    const int per_run = g.p2 >> 2;
    for (int q = tid; q < (g.P >> 2); q += RL_THREADS) {
      const int run = q / per_run, w = q - run * per_run, a0 = run / g.p1, a1 = run - a0 * g.p1;
      tgt4[q] = *reinterpret_cast<const f32x4*>(base + ((long)a0 * g.S1 + a1) * g.S2 + 4 * w);
    }
  } else {
    for (int e = tid; e < g.P; e += RL_THREADS) {
      const int run = e / g.p2, a2 = e - run * g.p2, a0 = run / g.p1, a1 = run - a0 * g.p1;
      tgt[e] = base[((long)a0 * g.S1 + a1) * g.S2 + a2];
    }
  }
  for (int e = g.P + tid; e < g.P8; e += RL_THREADS) tgt[e] = 0.f;
  __syncthreads();
  double mean = 0.0, inv_std = 1.0;
  if (norm_pix) {
    double s = 0.0;
    for (int e = tid; e < g.P; e += RL_THREADS) s += (double)tgt[e];
    mean = block_sum(s, red) / (double)g.P;
    double q = 0.0;
    for (int e = tid; e < g.P; e += RL_THREADS) { const double dv = (double)tgt[e] - mean; q += dv * dv; }
    const double var = block_sum(q, red) / (double)(g.P - 1);
    inv_std = 1.0 / sqrt(var + 1e-6);
  }
  double term = 0.0;
#pragma unroll
  for (int j = 0; j < RL_GROUPS; ++j) {
    const int q = tid + j * RL_THREADS, c = 8 * q;
    if (c >= g.P8) break;
    r16x8 out = zero8;
    const f32x4 ta = tgt4[2 * q], tb = tgt4[2 * q + 1];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (c + k < g.P) {
        const double tv = ((double)(k < 4 ? ta[k] : tb[k - 4]) - mean) * inv_std;
        const double diff = (double)(k < 4 ? pa[j][k] : pb[j][k - 4]) - tv;
        double dv;
        if (kind == 0) { term += fabs(diff); dv = diff > 0.0 ? gscale : (diff < 0.0 ? -gscale : diff); }      // (diff == 0: 0; NaN stays NaN)
        else { term += diff * diff; dv = gscale * diff; }
        out[k] = cvt1_once<T>(dv);
      }
    }
    *reinterpret_cast<r16x8*>(drow + c) = out;
  }
  for (int q = (g.P8 >> 3) + tid; q < groups_row; q += RL_THREADS) *reinterpret_cast<r16x8*>(drow + 8 * q) = zero8;      // the columns behind the patch
  const double row_term = block_sum(term, red);
  if (tid == 0) partials[r] = row_term * inv_count;
}

// loss[0] = the sum of partials[0, R) in index order, in double, stored as fp32.  One workgroup: all threads stage a chunk in LDS, thread 0 adds it up.
constexpr int RS_CHUNK = 2048;
__global__ __launch_bounds__(256) void recon_sum_kernel(const double* __restrict__ partials, long R, float* __restrict__ loss) {
  __shared__ double buf[RS_CHUNK];
  double s = 0.0;
  for (long r0 = 0; r0 < R; r0 += RS_CHUNK) {
    const int len = (int)((R - r0 < RS_CHUNK) ? R - r0 : RS_CHUNK);
    for (int k = threadIdx.x; k < len; k += 256) buf[k] = partials[r0 + k];
    __syncthreads();
    if (threadIdx.x == 0)       // (reading eight values ahead of the adds, or the next eight under them, changed nothing measurable: 9 ns per add either way)
      for (int k = 0; k < len; ++k) s += buf[k];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)s;
}

// ------------------------------------------------------------------------------------------------ token-gradient seed
constexpr int TS_THREADS = 256;

// Workgroup w takes the rows w, w + gridDim.x, ...: g = dtokens, g16 = cvt(dtokens * mask) with the dropout mask of the dense [M, d]
// tensor (element index row d + col, as nv_ln_bwd applies it), and partials[w, :] = the workgroup's column sums of dtokens * mask.
template <typename T>
__global__ __launch_bounds__(TS_THREADS) void token_grad_seed_kernel(const float* __restrict__ dtokens, int M, int d, float* __restrict__ g,
                                                                     r16* __restrict__ g16, float* __restrict__ partials, DropCfg drop) {
  for (int c = 4 * threadIdx.x; c < d; c += 4 * TS_THREADS) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int row = blockIdx.x; row < M; row += gridDim.x) {
      const long off = (long)row * d + c;
      f32x4 v = *reinterpret_cast<const f32x4*>(dtokens + off);
      *reinterpret_cast<f32x4*>(g + off) = v;
      if (drop.thresh) v *= drop_factor4(drop, (unsigned long long)off);
      *reinterpret_cast<r16x4*>(g16 + off) = cvt4<T>(v[0], v[1], v[2], v[3]);
      acc += v;
    }
    if (partials) *reinterpret_cast<f32x4*>(partials + (long)blockIdx.x * d + c) = acc;
  }
}

int mim_geom(const char* who, const int* grid3, int unit, MimGeom& g) {
  NV_CHECK_ARG(grid3 && grid3[0] > 0 && grid3[1] > 0 && grid3[2] > 0 && unit > 0, "%s: the patch grid and the mask unit must be positive", who);
  NV_CHECK_ARG(grid3[0] % unit == 0 && grid3[1] % unit == 0 && grid3[2] % unit == 0, "%s: the mask unit %d does not divide the patch grid %d x %d x %d", who, unit,
               grid3[0], grid3[1], grid3[2]);
  NV_CHECK_ARG((long)grid3[0] * grid3[1] * grid3[2] <= ML_MAX_CELLS, "%s: %ld patches, the kernel takes at most %d (16^3)", who,
               (long)grid3[0] * grid3[1] * grid3[2], ML_MAX_CELLS);
  g = MimGeom{grid3[0], grid3[1], grid3[2], unit, grid3[0] / unit, grid3[1] / unit, grid3[2] / unit};
  NV_CHECK_ARG(g.U0 * g.U1 * g.U2 >= 2, "%s: one mask unit covers the whole grid - nothing could stay visible", who);
  return NV_OK;
}
}  // namespace

extern "C" int nv_mim_masked_count(const int* grid3, int unit, double ratio) {
  MimGeom g;
  if (mim_geom("nv_mim_masked_count", grid3, unit, g)) return NV_ERR_ARG;
  NV_CHECK_ARG(ratio > 0.0 && ratio < 1.0, "nv_mim_masked_count: mask ratio %g outside (0, 1)", ratio);
  const int U = g.U0 * g.U1 * g.U2;
  int mu = (int)floor(ratio * (double)U + 0.5);
  mu = mu < 1 ? 1 : (mu > U - 1 ? U - 1 : mu);
  return mu * unit * unit * unit;
}

extern "C" int nv_mim_labels(unsigned long seed, unsigned long step, int rank, int B, const int* grid3, int unit, int* labels, void* stream) {
  NV_CHECK_ARG(labels && B > 0 && rank >= 0, "nv_mim_labels: bad arguments (null labels, B not positive, or a negative rank)");
  MimGeom g;
  if (const int rc = mim_geom("nv_mim_labels", grid3, unit, g)) return rc;
  NV_CHECK_ARG(nv_aligned(labels, 4), "nv_mim_labels: labels 4-byte aligned");
  hipLaunchKernelGGL(mim_labels_kernel, dim3(B), dim3(ML_THREADS), 0, (hipStream_t)stream, (uint64_t)seed, (uint64_t)rank, (uint64_t)step, g, labels);
  NV_CHECK_LAUNCH("nv_mim_labels");
  return NV_OK;
}

extern "C" int nv_recon_loss(const float* pred, long ldp, const float* x, int B, const int* size3, const int* patch3, const int* labels, int m, int kind,
                             int norm_pix, float loss_scale, void* dpred, long ldd, double* partials, float* loss, void* stream) {
  NV_CHECK_ARG(pred && x && size3 && patch3 && labels && dpred && partials && loss && B > 0, "nv_recon_loss: bad arguments (null pointer, or B not positive)");
  ReconGeom g;
  g.B = B; g.S0 = size3[0]; g.S1 = size3[1]; g.S2 = size3[2]; g.p0 = patch3[0]; g.p1 = patch3[1]; g.p2 = patch3[2];
  NV_CHECK_ARG(g.S0 > 0 && g.S1 > 0 && g.S2 > 0 && g.p0 > 0 && g.p1 > 0 && g.p2 > 0, "nv_recon_loss: volume and patch extents must be positive");
  NV_CHECK_ARG(g.S0 % g.p0 == 0 && g.S1 % g.p1 == 0 && g.S2 % g.p2 == 0, "nv_recon_loss: volume %d x %d x %d is not a whole number of %d x %d x %d patches", g.S0,
               g.S1, g.S2, g.p0, g.p1, g.p2);
  g.G0 = g.S0 / g.p0; g.G1 = g.S1 / g.p1;
  const long N = (long)g.G0 * g.G1 * (g.S2 / g.p2), P = (long)g.p0 * g.p1 * g.p2;
  NV_CHECK_ARG(N <= ML_MAX_CELLS && P <= RL_MAX_P, "nv_recon_loss: %ld patches of %ld voxels, the kernel takes at most %d of %d", N, P, ML_MAX_CELLS, RL_MAX_P);
  g.N = (int)N; g.n = g.N + 1; g.P = (int)P; g.P8 = (int)((P + 7) / 8 * 8);
  NV_CHECK_ARG(m >= 1 && m <= g.N, "nv_recon_loss: %d masked patches per volume outside [1, %d]", m, g.N);
  NV_CHECK_ARG(kind == NV_RECON_L1 || kind == NV_RECON_L2, "nv_recon_loss: kind %d is neither NV_RECON_L1 nor NV_RECON_L2", kind);
  NV_CHECK_ARG(!norm_pix || g.P >= 2, "nv_recon_loss: norm_pix needs patches of at least two voxels");
  NV_CHECK_ARG(isfinite(loss_scale) && loss_scale > 0.f, "nv_recon_loss: loss_scale %g must be finite and positive", (double)loss_scale);
  NV_CHECK_ARG(ldp >= g.P8 && ldp % 4 == 0 && nv_aligned16(pred), "nv_recon_loss: pred 16-byte aligned with ldp = %ld a multiple of 4 and at least %d", ldp, g.P8);
  NV_CHECK_ARG(ldd >= g.P8 && ldd % 8 == 0 && nv_aligned16(dpred), "nv_recon_loss: dpred 16-byte aligned with ldd = %ld a multiple of 8 and at least %d", ldd, g.P8);
  NV_CHECK_ARG(nv_aligned(x, 4) && nv_aligned(labels, 4) && nv_aligned(partials, 8) && nv_aligned(loss, 4), "nv_recon_loss: element-aligned buffers");
  const long rows = (long)B * g.n;
  NV_CHECK_ARG(rows < (1L << 31), "nv_recon_loss: B n too large");
  const double count = (double)B * (double)m * (double)g.P;
  const double inv_count = 1.0 / count, gscale = (kind == NV_RECON_L2 ? 2.0 : 1.0) * (double)loss_scale / count;
  const bool vec = nv_aligned16(x) && g.S2 % 4 == 0 && g.p2 % 4 == 0;       // every run of every patch then starts on a 16-byte boundary
  hipStream_t s = (hipStream_t)stream;
  NV_DISPATCH_OPERAND(T,
    if (vec) hipLaunchKernelGGL((recon_loss_kernel<T, true>), dim3((unsigned)rows), dim3(RL_THREADS), 0, s, pred, ldp, x, g, labels, m, kind, norm_pix, inv_count,
                                gscale, (r16*)dpred, ldd, partials);
    else hipLaunchKernelGGL((recon_loss_kernel<T, false>), dim3((unsigned)rows), dim3(RL_THREADS), 0, s, pred, ldp, x, g, labels, m, kind, norm_pix, inv_count,
                            gscale, (r16*)dpred, ldd, partials));
  NV_CHECK_LAUNCH("nv_recon_loss");
  hipLaunchKernelGGL(recon_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, rows, loss);
  NV_CHECK_LAUNCH("nv_recon_loss (sum)");
  return NV_OK;
}

static int token_seed_blocks(int M) { return M < 256 ? M : 256; }
extern "C" long nv_token_grad_seed_workspace_bytes(int M, int d) { return M > 0 && d > 0 ? (long)token_seed_blocks(M) * d * (long)sizeof(float) : -1; }
extern "C" int nv_token_grad_seed_rows(int M) { return M > 0 ? token_seed_blocks(M) : -1; }

extern "C" int nv_token_grad_seed(const float* dtokens, int M, int d, float* g, void* g16, float* partials, long partial_bytes, unsigned long drop_seed,
                                  float drop_p, void* stream) {
  NV_CHECK_ARG(dtokens && g && g16 && M > 0 && d > 0 && d % 4 == 0, "nv_token_grad_seed: bad arguments (null pointer, M < 1, or d no positive multiple of 4)");
  NV_CHECK_ARG(nv_aligned16(dtokens) && nv_aligned16(g) && nv_aligned(g16, 8) && nv_aligned16(partials), "nv_token_grad_seed: dtokens, g and partials 16-byte aligned, g16 8-byte");
  NV_CHECK_ARG(!partials || partial_bytes >= nv_token_grad_seed_workspace_bytes(M, d), "nv_token_grad_seed: partials too small (%ld < %ld bytes)", partial_bytes,
               nv_token_grad_seed_workspace_bytes(M, d));
  const DropCfg drop = make_drop(drop_seed, drop_p);
  NV_DISPATCH_OPERAND(T, hipLaunchKernelGGL((token_grad_seed_kernel<T>), dim3(token_seed_blocks(M)), dim3(TS_THREADS), 0, (hipStream_t)stream, dtokens, M, d, g,
                                            (r16*)g16, partials, drop));
  NV_CHECK_LAUNCH("nv_token_grad_seed");
  return NV_OK;
}
