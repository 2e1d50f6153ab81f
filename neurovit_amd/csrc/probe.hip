// A linear probe over the frozen-feature bank: column statistics (nv_probe_stats), the fused logits + loss + weight-gradient pass
// (nv_probe_grad), the Adam step (nv_probe_step) and the prediction (nv_probe_predict).  The definitions are in the header.  Nothing here
// reads back, nothing uses atomics; every sum has one fixed order, so the bits reproduce from run to run and do not depend on the grid.
#include <math.h>

#include "eval_common.h"

// Every fp32 / fp64 operation below is rounded on its own: through the operators of eval_common.h (which says why the toolchain's rounded
// intrinsics do not do), and under the same mode for what is written out in place.  The matrix products are MFMA builtins and are not affected.
#pragma clang fp contract(off)

namespace {

constexpr int PT = 32;                      // rows of a tile: the k extent of the weight-gradient product, two 16-row blocks of the logits
constexpr int PCH = NV_PROBE_CHUNK;         // rows of a chunk: one [M, d] partial in the workspace
constexpr int PMAXM = NV_PROBE_MAX_M;
static_assert(PCH % PT == 0, "a chunk is a whole number of tiles");

struct ProbeArgs {
  const float* X;
  long ldx;
  int N, d;
  const float* mean;
  const float* rstd;
  const float* W;
  const float* b;
  int H, C, M, task;
  const int* labels;
  const float* cw;
  const float* targets;
  const float* tmean;
  const float* tstd;
  float* part;            // [nchunks][M][d]
  double* lossc;          // [nchunks][PMAXM]
  double* dbc;            // [nchunks][PMAXM]
  int nchunks;
  float* logits;          // the prediction's outputs
  long ldl;
  float* probs;
  long ldp;
};

// fp32 softmax of one head's C logits (max-subtracted, expf, the sum in ascending column order): returns the sum, *mx the maximum
__device__ __forceinline__ float probe_softmax_sum(const float* lg, int C, float* mx) {
  float m = lg[0];
  for (int k = 1; k < C; ++k) m = fmaxf(m, lg[k]);
  float s = 0.f;
  for (int k = 0; k < C; ++k) s = radd(s, expf(rsub(lg[k], m)));
  *mx = m;
  return s;
}

// Workgroup = 4 waves; a tile = 32 rows of Z = (X - mean) rstd, staged ONCE in LDS ([32][64 NB + 16] floats: the 16 spare columns put the four
// row groups of an MFMA operand read on distinct banks) and read by both products.
//   logits [32, M] = Z W^T: the 64 NB columns are divided into four quarters, wave w contracts its quarter (W comes from global memory: M rows
//     of d floats, cache-resident); the four partial tiles meet in LDS and are added as (p0 + p1) + (p2 + p3), then the bias.
//   loss and dlogits per (row, head), in place over the logits.
//   dW [M, 64 NB] += dlogits^T Z: wave w owns the columns of its quarter, MT x NB accumulator blocks that live in registers across the tiles
//     of a chunk; k = the tile's rows, ascending.
// PREDICT: the logits (and the softmax) are written out instead; nothing else runs.
template <int MT, int NB, bool PREDICT>
__global__ __launch_bounds__(256) void probe_tile_kernel(ProbeArgs a) {
  constexpr int DP = NB * 64, LDZ = DP + 16, MP = 16 * MT, GLD = MP + 1, WC = NB * 16;
  extern __shared__ __attribute__((aligned(16))) float psm[];
  float* zt = psm;                        // [PT][LDZ]
  float* pl = zt + PT * LDZ;              // [4][PT][GLD] the waves' partial logits
  float* gl = pl + 4 * PT * GLD;          // [PT][GLD] logits, then dlogits
  float* ll = gl + PT * GLD;              // [PT][GLD] loss cells
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, g = lane >> 4;
  for (int chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
    const int cbeg = chunk * PCH, cend = min(cbeg + PCH, a.N);
    f32x4 acc[MT][NB];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[mt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    double accL = 0.0, accB = 0.0;
    for (int r0 = cbeg; r0 < cend; r0 += PT) {
      // ---- stage the tile (rows past the chunk's end and columns past d are zeros): eight loads in flight per thread, from clamped
      // addresses and without a branch between them; what lies outside the tile is replaced by zeros behind the loads
      constexpr int SB = 2 * NB < 8 ? 2 * NB : 8;
#pragma unroll
      for (int it0 = 0; it0 < 2 * NB; it0 += SB) {
        f32x4 v[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int e = tid + 256 * (it0 + u), row = min(r0 + e / (NB * 16), cend - 1), c4 = min((e % (NB * 16)) * 4, a.d - 4);
          v[u] = *reinterpret_cast<const f32x4*>(a.X + (long)row * a.ldx + c4);
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
          const int e = tid + 256 * (it0 + u), r = e / (NB * 16), c4 = (e % (NB * 16)) * 4;
          if (a.mean) {
            const int cc = min(c4, a.d - 4);
            const f32x4 mu = *reinterpret_cast<const f32x4*>(a.mean + cc), rs = *reinterpret_cast<const f32x4*>(a.rstd + cc);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[u][j] = rmul(rsub(v[u][j], mu[j]), rs[j]);
          }
          const bool inside = r0 + r < cend && c4 < a.d;
          *reinterpret_cast<f32x4*>(zt + r * LDZ + c4) = inside ? v[u] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      __syncthreads();
      // ---- logits: this wave's quarter of the columns
      f32x4 la[2][MT];
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int ct = 0; ct < MT; ++ct) la[rb][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < NB; ++s) {
        const int kb = wid * WC + 16 * s + 4 * g;
        f32x4 zf[2], wf[MT];
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) zf[rb] = *reinterpret_cast<const f32x4*>(zt + (16 * rb + i) * LDZ + kb);
#pragma unroll
        for (int ct = 0; ct < MT; ++ct) {
          const int col = 16 * ct + i;
          wf[ct] = (col < a.M && kb < a.d) ? *reinterpret_cast<const f32x4*>(a.W + (long)col * a.d + kb) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int ct = 0; ct < MT; ++ct) la[rb][ct] = mfma4(wf[ct][t], zf[rb][t], la[rb][ct]);
      }
      // register r of block (rb, ct) holds the partial logit of row 16 rb + i, column 16 ct + 4 g + r
#pragma unroll
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int ct = 0; ct < MT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) pl[(wid * PT + 16 * rb + i) * GLD + 16 * ct + 4 * g + r] = la[rb][ct][r];
      __syncthreads();
      for (int e = tid; e < PT * MP; e += 256) {
        const int r = e / MP, m = e % MP;
        float v = radd(radd(pl[r * GLD + m], pl[(PT + r) * GLD + m]), radd(pl[(2 * PT + r) * GLD + m], pl[(3 * PT + r) * GLD + m]));
        v = m < a.M ? radd(v, a.b[m]) : 0.f;
        gl[r * GLD + m] = v;
        ll[r * GLD + m] = 0.f;
      }
      __syncthreads();
      if constexpr (PREDICT) {
        for (int e = tid; e < PT * a.M; e += 256) {
          const int r = e / a.M, m = e % a.M, row = r0 + r;
          if (row < cend) a.logits[(long)row * a.ldl + m] = gl[r * GLD + m];
        }
        if (a.probs) {
          for (int t = tid; t < PT * a.H; t += 256) {
            const int r = t / a.H, h = t % a.H, row = r0 + r;
            if (row >= cend) continue;
            const float* lg = gl + r * GLD + h * a.C;
            float mx;
            const float s = probe_softmax_sum(lg, a.C, &mx);
            for (int k = 0; k < a.C; ++k) a.probs[(long)row * a.ldp + h * a.C + k] = rdiv(expf(rsub(lg[k], mx)), s);
          }
        }
        continue;      // (the next tile's two barriers stand between these reads and the next writes of gl)
      }
      // ---- loss and dlogits, in place
      if (a.task == NV_PROBE_CLASSIFICATION) {
        for (int t = tid; t < PT * a.H; t += 256) {
          const int r = t / a.H, h = t % a.H, row = r0 + r;
          float* lg = gl + r * GLD + h * a.C;
          int y = -1;
          if (row < cend) {
            y = a.labels[row];
            if (!valid_label(y, a.C)) y = -1;
          }
          if (y < 0) {
            for (int k = 0; k < a.C; ++k) lg[k] = 0.f;
            continue;
          }
          float mx;
          const float s = probe_softmax_sum(lg, a.C, &mx);
          const float c = a.cw ? a.cw[y] : 1.f;
          ll[r * GLD + h * a.C] = rmul(c, rsub(logf(s), rsub(lg[y], mx)));
          for (int k = 0; k < a.C; ++k) {
            const float p = rdiv(expf(rsub(lg[k], mx)), s);
            lg[k] = rmul(c, rsub(p, k == y ? 1.f : 0.f));
          }
        }
      } else {
        for (int t = tid; t < PT * a.M; t += 256) {
          const int r = t / a.M, m = t % a.M, row = r0 + r, k = m % a.C;
          float gv = 0.f, lv = 0.f;
          if (row < cend) {
            const float y = a.targets[(long)row * a.C + k];
            if (y == y) {
              const float ts = rdiv(rsub(y, a.tmean ? a.tmean[k] : 0.f), a.tstd ? a.tstd[k] : 1.f);
              const float rr = rsub(gl[r * GLD + m], ts);
              gv = rmul(2.f, rr);
              lv = rmul(rr, rr);
            }
          }
          gl[r * GLD + m] = gv;
          ll[r * GLD + m] = lv;
        }
      }
      __syncthreads();
      if (tid < a.M) {      // the bias gradient and the loss of column tid: the tile's rows in ascending order, in double
        for (int r = 0; r < PT; ++r) {
          accB = dadd(accB, (double)gl[r * GLD + tid]);
          accL = dadd(accL, (double)ll[r * GLD + tid]);
        }
      }
      // ---- dW += dlogits^T Z over this wave's columns
#pragma unroll
      for (int kk = 0; kk < PT / 4; ++kk) {
        float gv[MT], zv[NB];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) gv[mt] = gl[(4 * kk + g) * GLD + 16 * mt + i];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) zv[nb] = zt[(4 * kk + g) * LDZ + wid * WC + 16 * nb + i];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) acc[mt][nb] = mfma4(gv[mt], zv[nb], acc[mt][nb]);
      }
      __syncthreads();      // the tile is consumed before the next one lands on it
    }
    if constexpr (!PREDICT) {
      // register r of block (mt, nb) holds dW[16 mt + 4 g + r][wid WC + 16 nb + i]
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = 16 * mt + 4 * g + r, col = wid * WC + 16 * nb + i;
            if (m < a.M && col < a.d) a.part[((long)chunk * a.M + m) * a.d + col] = acc[mt][nb][r];
          }
      if (tid < a.M) {
        a.lossc[(long)chunk * PMAXM + tid] = accL;
        a.dbc[(long)chunk * PMAXM + tid] = accB;
      }
    }
  }
}

// The chunk partials in ascending chunk order, in double, rounded once.  Blocks 0 .. ceil(M d / 256) - 1: dW; the last block: db and loss.
__global__ __launch_bounds__(256) void probe_reduce_kernel(const float* __restrict__ part, const double* __restrict__ lossc, const double* __restrict__ dbc,
                                                           int nchunks, int M, int d, const float* __restrict__ W, nv_probe_heads hd, int task,
                                                           const double* __restrict__ denom, float* __restrict__ dW, float* __restrict__ db,
                                                           float* __restrict__ loss) {
  const int tid = threadIdx.x;
  const long md = (long)M * d;
  if (blockIdx.x + 1 < gridDim.x) {
    const long idx = (long)blockIdx.x * 256 + tid;
    if (idx >= md) return;
    const int m = (int)(idx / d);
    double s = 0.0;
    int c = 0;
    for (; c + 16 <= nchunks; c += 16) {      // sixteen loads in flight, added in ascending chunk order
      float t[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) t[u] = part[(long)(c + u) * md + idx];
#pragma unroll
      for (int u = 0; u < 16; ++u) s = dadd(s, (double)t[u]);
    }
    for (; c < nchunks; ++c) s = dadd(s, (double)part[(long)c * md + idx]);
    const double D = denom[task == NV_PROBE_REGRESSION ? m % hd.C : 0];
    const double data = D > 0.0 ? s / D : 0.0;
    dW[idx] = (float)dadd(data, dmul((double)hd.l2[m / hd.C], (double)W[idx]));
    return;
  }
  if (tid < M) {
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s = dadd(s, dbc[(long)c * PMAXM + tid]);
    const double D = denom[task == NV_PROBE_REGRESSION ? tid % hd.C : 0];
    db[tid] = (float)(D > 0.0 ? s / D : 0.0);
  }
  if (tid < hd.H) {
    double L = 0.0;
    for (int k = 0; k < hd.C; ++k) {
      double s = 0.0;
      for (int c = 0; c < nchunks; ++c) s = dadd(s, lossc[(long)c * PMAXM + tid * hd.C + k]);
      const double D = denom[task == NV_PROBE_REGRESSION ? k : 0];
      L = dadd(L, D > 0.0 ? s / D : 0.0);
    }
    loss[tid] = (float)L;
  }
}

// Adam, every fp32 operation rounded on its own.  One thread per element of W (blocks 0 .. ceil(M d / 256) - 1) or of b (the last block).
__device__ __forceinline__ void probe_adam(float& p, float g, float& m, float& v, float step, float b1, float b2, float omb1, float omb2, float bc2s, float eps) {
  m = radd(rmul(b1, m), rmul(omb1, g));
  v = radd(rmul(b2, v), rmul(rmul(omb2, g), g));
  // the root in double, rounded once: the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits) whatever the fp32 sqrt of the toolchain does
  const float den = radd(rdiv((float)sqrt((double)v), bc2s), eps);
  p = rsub(p, rmul(step, rdiv(m, den)));
}

__global__ __launch_bounds__(256) void probe_step_kernel(float* __restrict__ W, float* __restrict__ b, const float* __restrict__ dW, const float* __restrict__ db,
                                                         float* __restrict__ mW, float* __restrict__ vW, float* __restrict__ mb, float* __restrict__ vb, int M, int d,
                                                         nv_probe_heads hd, float b1, float b2, float omb1, float omb2, float bc2s, float eps) {
  const int tid = threadIdx.x;
  if (blockIdx.x + 1 < gridDim.x) {
    const long idx = (long)blockIdx.x * 256 + tid;
    if (idx >= (long)M * d) return;
    float p = W[idx], m = mW[idx], v = vW[idx];
    probe_adam(p, dW[idx], m, v, hd.step[(int)(idx / d) / hd.C], b1, b2, omb1, omb2, bc2s, eps);
    W[idx] = p;
    mW[idx] = m;
    vW[idx] = v;
    return;
  }
  if (tid < M) {
    float p = b[tid], m = mb[tid], v = vb[tid];
    probe_adam(p, db[tid], m, v, hd.step[tid / hd.C], b1, b2, omb1, omb2, bc2s, eps);
    b[tid] = p;
    mb[tid] = m;
    vb[tid] = v;
  }
}

// ------------------------------------------------------------------------------------------------ statistics
// pass 0: per (chunk, column) the sum and the count of the observed cells; pass 1: the sum of the squared deviations from the fp64 mean.
__global__ __launch_bounds__(256) void probe_stats_partial_kernel(const float* __restrict__ X, long ldx, int N, int d, int skip_nan, int pass,
                                                                  const double* __restrict__ meand, double* __restrict__ psum, double* __restrict__ pcnt) {
  const int col = blockIdx.x * 256 + threadIdx.x, chunk = blockIdx.y;
  if (col >= d) return;
  const int rbeg = chunk * PCH, rend = min(rbeg + PCH, N);
  const double mu = pass ? meand[col] : 0.0;
  double s = 0.0, n = 0.0;
  for (int row = rbeg; row < rend; ++row) {
    const float x = X[(long)row * ldx + col];
    if (skip_nan && x != x) continue;
    if (pass == 0) {
      s = dadd(s, (double)x);
      n += 1.0;
    } else {
      const double dx = dsub((double)x, mu);
      s = dadd(s, dmul(dx, dx));
    }
  }
  psum[(long)chunk * d + col] = s;
  if (pass == 0) pcnt[(long)chunk * d + col] = n;
}

__global__ __launch_bounds__(256) void probe_stats_finish_kernel(int pass, int nchunks, int d, const double* __restrict__ psum, const double* __restrict__ pcnt,
                                                                 double* __restrict__ meand, double* __restrict__ cntd, float eps, float* __restrict__ mean,
                                                                 float* __restrict__ rstd, float* __restrict__ sd, double* __restrict__ count) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double s = 0.0;
  for (int c = 0; c < nchunks; ++c) s = dadd(s, psum[(long)c * d + col]);
  if (pass == 0) {
    double n = 0.0;
    for (int c = 0; c < nchunks; ++c) n += pcnt[(long)c * d + col];
    cntd[col] = n;
    meand[col] = n > 0.0 ? s / n : 0.0;
    return;
  }
  const double n = cntd[col], var = n > 0.0 ? s / n : 0.0;
  if (mean) mean[col] = (float)meand[col];
  if (rstd) rstd[col] = var > 0.0 ? (float)(1.0 / sqrt(dadd(var, (double)eps))) : 0.f;
  if (sd) sd[col] = (float)sqrt(var);
  if (count) count[col] = n;
}

// one workgroup: thread t forms the partials of the chunks t, t + 256, ...; thread 0 adds them in ascending chunk order
__global__ __launch_bounds__(256) void probe_denom_kernel(const int* __restrict__ labels, int N, int C, const float* __restrict__ cw, int nchunks,
                                                          double* __restrict__ lp, double* __restrict__ denom) {
  for (int c = threadIdx.x; c < nchunks; c += 256) {
    const int rbeg = c * PCH, rend = min(rbeg + PCH, N);
    double s = 0.0;
    for (int row = rbeg; row < rend; ++row) {
      const int y = labels[row];
      if (valid_label(y, C)) s = dadd(s, cw ? (double)cw[y] : 1.0);
    }
    lp[c] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int c = 0; c < nchunks; ++c) t = dadd(t, lp[c]);
    denom[0] = t;
  }
}

// ------------------------------------------------------------------------------------------------ host side
int probe_chunks(int N) { return (N + PCH - 1) / PCH; }

int probe_nb(int d) {      // the instantiated widths: 64 NB columns cover d
  const int need = (d + 63) / 64;
  const int have[6] = {1, 2, 4, 8, 12, 16};
  for (int k = 0; k < 6; ++k)
    if (have[k] >= need) return have[k];
  return 0;
}

size_t probe_lds_bytes(int MT, int NB) { return (size_t)(PT * (NB * 64 + 16) + 6 * PT * (16 * MT + 1)) * sizeof(float); }
static_assert((size_t)(PT * (16 * 64 + 16) + 6 * PT * (16 * 2 + 1)) * sizeof(float) <= 160 * 1024, "LDS budget");

template <int MT, int NB, bool PREDICT>
int probe_launch_one(const ProbeArgs& a, int grid, hipStream_t s) {
  const size_t lds = probe_lds_bytes(MT, NB);
  if (lds > 64 * 1024) {
    static bool allowed = false;
    if (int rc = allow_lds(probe_tile_kernel<MT, NB, PREDICT>, (int)lds, allowed, PREDICT ? "nv_probe_predict" : "nv_probe_grad")) return rc;
  }
  hipLaunchKernelGGL((probe_tile_kernel<MT, NB, PREDICT>), dim3(grid), dim3(256), lds, s, a);
  return NV_OK;
}

template <bool PREDICT>
int probe_launch(const ProbeArgs& a, int grid, hipStream_t s) {
  const int MT = a.M > 16 ? 2 : 1, NB = probe_nb(a.d);
#define NV_PROBE_CASE(mt, nb) \
  if (MT == mt && NB == nb) return probe_launch_one<mt, nb, PREDICT>(a, grid, s)
  NV_PROBE_CASE(1, 1); NV_PROBE_CASE(1, 2); NV_PROBE_CASE(1, 4); NV_PROBE_CASE(1, 8); NV_PROBE_CASE(1, 12); NV_PROBE_CASE(1, 16);
  NV_PROBE_CASE(2, 1); NV_PROBE_CASE(2, 2); NV_PROBE_CASE(2, 4); NV_PROBE_CASE(2, 8); NV_PROBE_CASE(2, 12); NV_PROBE_CASE(2, 16);
#undef NV_PROBE_CASE
  return NV_OK;      // (probe_nb covers every d that the entry points let through)
}

bool probe_shape_ok(int N, int d, int M) { return N > 0 && d >= 4 && d <= NV_PROBE_MAX_D && (d % 4) == 0 && M >= 1 && M <= PMAXM; }

int probe_check_heads(const char* who, const nv_probe_heads* hd) {
  NV_CHECK_ARG(hd && hd->struct_size == (int)sizeof(nv_probe_heads), "%s: nv_probe_heads is NULL or its struct_size = %d, this library's nv_probe_heads has %d bytes", who,
               hd ? hd->struct_size : 0, (int)sizeof(nv_probe_heads));
  NV_CHECK_ARG(hd->H >= 1 && hd->C >= 1 && hd->H <= PMAXM && hd->C <= PMAXM && hd->H * hd->C <= PMAXM, "%s: H=%d heads of C=%d columns: H * C must lie in [1, %d]", who,
               hd->H, hd->C, PMAXM);
  for (int h = 0; h < hd->H; ++h) NV_CHECK_ARG(hd->l2[h] >= 0.f && hd->l2[h] < INFINITY, "%s: l2[%d] = %g must be finite and >= 0", who, h, (double)hd->l2[h]);
  return NV_OK;
}

}  // namespace

extern "C" long nv_probe_stats_workspace_bytes(int N, int d) {
  if (N <= 0 || d < 0) return 0;
  const long nc = probe_chunks(N);
  return (2 * nc * d + 2L * d + nc) * (long)sizeof(double);
}

extern "C" int nv_probe_stats(const float* X, long ldx, int N, int d, int skip_nan, float eps, float* mean, float* rstd, float* std, double* count,
                              const int* labels, int C, const float* class_weight, double* denom, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(N > 0 && d >= 0 && (X || labels), "nv_probe_stats: bad shape N=%d d=%d, or neither X nor labels", N, d);
  NV_CHECK_ARG((X != nullptr) == (d > 0), "nv_probe_stats: X and d=%d are given together (X == NULL with d == 0 when only denom is wanted)", d);
  NV_CHECK_ARG(!X || (ldx >= d && (mean || rstd || std || count)), "nv_probe_stats: ldx=%ld must cover d=%d, and one of mean / rstd / std / count is wanted", ldx, d);
  NV_CHECK_ARG(eps >= 0.f && eps < INFINITY, "nv_probe_stats: eps = %g must be finite and >= 0", (double)eps);
  NV_CHECK_ARG((labels != nullptr) == (denom != nullptr), "nv_probe_stats: labels and denom are given together or not at all");
  NV_CHECK_ARG(!labels || C >= 1, "nv_probe_stats: labels need C=%d >= 1", C);
  NV_CHECK_ARG(labels || !class_weight, "nv_probe_stats: class_weight without labels");
  NV_CHECK_ARG(nv_aligned(X, 4) && nv_aligned(mean, 4) && nv_aligned(rstd, 4) && nv_aligned(std, 4) && nv_aligned(count, 8) && nv_aligned(labels, 4) &&
                   nv_aligned(class_weight, 4) && nv_aligned(denom, 8),
               "nv_probe_stats: float and int arrays 4-byte aligned, count and denom 8-byte aligned");
  const long need = nv_probe_stats_workspace_bytes(N, d);
  NV_CHECK_ARG(workspace && ws_bytes >= need && nv_aligned(workspace, 8), "nv_probe_stats: the workspace needs %ld bytes (nv_probe_stats_workspace_bytes), 8-byte aligned, got %ld", need,
               workspace ? ws_bytes : 0L);
  const int nc = probe_chunks(N);
  NV_CHECK_ARG(nc <= 65535, "nv_probe_stats: N=%d is more than 65535 chunks of %d rows", N, PCH);
  hipStream_t s = (hipStream_t)stream;
  double* psum = (double*)workspace;
  double* pcnt = psum + (long)nc * d;
  double* meand = pcnt + (long)nc * d;
  double* cntd = meand + d;
  double* lp = cntd + d;
  if (X) {
    const dim3 grid((d + 255) / 256, nc), fgrid((d + 255) / 256);
    hipLaunchKernelGGL(probe_stats_partial_kernel, grid, dim3(256), 0, s, X, ldx, N, d, skip_nan ? 1 : 0, 0, (const double*)meand, psum, pcnt);
    hipLaunchKernelGGL(probe_stats_finish_kernel, fgrid, dim3(256), 0, s, 0, nc, d, (const double*)psum, (const double*)pcnt, meand, cntd, eps, mean, rstd, std, count);
    hipLaunchKernelGGL(probe_stats_partial_kernel, grid, dim3(256), 0, s, X, ldx, N, d, skip_nan ? 1 : 0, 1, (const double*)meand, psum, pcnt);
    hipLaunchKernelGGL(probe_stats_finish_kernel, fgrid, dim3(256), 0, s, 1, nc, d, (const double*)psum, (const double*)pcnt, meand, cntd, eps, mean, rstd, std, count);
  }
  if (labels) hipLaunchKernelGGL(probe_denom_kernel, dim3(1), dim3(256), 0, s, labels, N, C, class_weight, nc, lp, denom);
  NV_CHECK_LAUNCH("nv_probe_stats");
  return NV_OK;
}

extern "C" long nv_probe_grad_workspace_bytes(int N, int d, int M) {
  if (!probe_shape_ok(N, d, M)) return 0;
  const long nc = probe_chunks(N);
  return nc * ((long)M * d * (long)sizeof(float) + 2L * PMAXM * (long)sizeof(double));
}

extern "C" int nv_probe_grad(const float* X, long ldx, int N, int d, const float* mean, const float* rstd, const float* W, const float* b,
                             const nv_probe_heads* heads, int task, const int* labels, const float* class_weight, const float* targets,
                             const float* target_mean, const float* target_std, const double* denom, float* dW, float* db, float* loss, int max_blocks,
                             void* workspace, long ws_bytes, void* stream) {
  if (int rc = probe_check_heads("nv_probe_grad", heads)) return rc;
  const int M = heads->H * heads->C;
  NV_CHECK_ARG(X && W && b && dW && db && loss && denom && N > 0, "nv_probe_grad: null pointer or N=%d", N);
  NV_CHECK_ARG(d >= 4 && d <= NV_PROBE_MAX_D && (d % 4) == 0, "nv_probe_grad: d=%d must be a multiple of 4 in [4, %d]", d, NV_PROBE_MAX_D);
  NV_CHECK_ARG(ldx >= d && (ldx % 4) == 0 && nv_aligned16(X) && nv_aligned16(W) && nv_aligned16(mean) && nv_aligned16(rstd),
               "nv_probe_grad: ldx=%ld must be a multiple of 4 with ldx >= d=%d; X, W, mean and rstd 16-byte aligned", ldx, d);
  NV_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "nv_probe_grad: mean and rstd are given together or not at all");
  NV_CHECK_ARG(task == NV_PROBE_CLASSIFICATION || task == NV_PROBE_REGRESSION, "nv_probe_grad: unknown task %d", task);
  if (task == NV_PROBE_CLASSIFICATION)
    NV_CHECK_ARG(labels && !targets && !target_mean && !target_std, "nv_probe_grad: classification takes labels, and no targets, target_mean or target_std");
  else
    NV_CHECK_ARG(targets && !labels && !class_weight, "nv_probe_grad: regression takes targets, and no labels or class_weight");
  NV_CHECK_ARG(nv_aligned(b, 4) && nv_aligned(labels, 4) && nv_aligned(class_weight, 4) && nv_aligned(targets, 4) && nv_aligned(target_mean, 4) &&
                   nv_aligned(target_std, 4) && nv_aligned(denom, 8) && nv_aligned(dW, 4) && nv_aligned(db, 4) && nv_aligned(loss, 4),
               "nv_probe_grad: float and int arrays 4-byte aligned, denom 8-byte aligned");
  NV_CHECK_ARG(max_blocks >= 0, "nv_probe_grad: max_blocks=%d must be >= 0 (0 = one workgroup per chunk)", max_blocks);
  const long need = nv_probe_grad_workspace_bytes(N, d, M);
  NV_CHECK_ARG(workspace && ws_bytes >= need && nv_aligned(workspace, 8), "nv_probe_grad: the workspace needs %ld bytes (nv_probe_grad_workspace_bytes), 8-byte aligned, got %ld", need,
               workspace ? ws_bytes : 0L);
  const int nc = probe_chunks(N);
  ProbeArgs a{};
  a.X = X; a.ldx = ldx; a.N = N; a.d = d; a.mean = mean; a.rstd = rstd; a.W = W; a.b = b;
  a.H = heads->H; a.C = heads->C; a.M = M; a.task = task;
  a.labels = labels; a.cw = class_weight; a.targets = targets; a.tmean = target_mean; a.tstd = target_std;
  a.lossc = (double*)workspace;
  a.dbc = a.lossc + (long)nc * PMAXM;
  a.part = (float*)(a.dbc + (long)nc * PMAXM);
  a.nchunks = nc;
  hipStream_t s = (hipStream_t)stream;
  if (int rc = probe_launch<false>(a, max_blocks > 0 && max_blocks < nc ? max_blocks : nc, s)) return rc;
  const int eb = (int)(((long)M * d + 255) / 256);
  hipLaunchKernelGGL(probe_reduce_kernel, dim3(eb + 1), dim3(256), 0, s, (const float*)a.part, (const double*)a.lossc, (const double*)a.dbc, nc, M, d, W, *heads, task,
                     denom, dW, db, loss);
  NV_CHECK_LAUNCH("nv_probe_grad");
  return NV_OK;
}

extern "C" int nv_probe_step(float* W, float* b, const float* dW, const float* db, float* mW, float* vW, float* mb, float* vb, int d,
                             const nv_probe_heads* heads, float beta1, float beta2, float one_minus_b1, float one_minus_b2, float bc2_sqrt, float eps,
                             void* stream) {
  if (int rc = probe_check_heads("nv_probe_step", heads)) return rc;
  const int M = heads->H * heads->C;
  NV_CHECK_ARG(W && b && dW && db && mW && vW && mb && vb, "nv_probe_step: null pointer");
  NV_CHECK_ARG(d >= 1 && d <= NV_PROBE_MAX_D, "nv_probe_step: d=%d outside [1, %d]", d, NV_PROBE_MAX_D);
  NV_CHECK_ARG(nv_aligned(W, 4) && nv_aligned(b, 4) && nv_aligned(dW, 4) && nv_aligned(db, 4) && nv_aligned(mW, 4) && nv_aligned(vW, 4) && nv_aligned(mb, 4) && nv_aligned(vb, 4),
               "nv_probe_step: every array 4-byte aligned");
  NV_CHECK_ARG(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && bc2_sqrt > 0.f && eps >= 0.f, "nv_probe_step: beta1=%g, beta2=%g in [0, 1), bc2_sqrt=%g > 0, eps=%g >= 0",
               (double)beta1, (double)beta2, (double)bc2_sqrt, (double)eps);
  for (int h = 0; h < heads->H; ++h) NV_CHECK_ARG(heads->step[h] == heads->step[h] && fabsf(heads->step[h]) < INFINITY, "nv_probe_step: step[%d] is not finite", h);
  const int eb = (int)(((long)M * d + 255) / 256);
  hipLaunchKernelGGL(probe_step_kernel, dim3(eb + 1), dim3(256), 0, (hipStream_t)stream, W, b, dW, db, mW, vW, mb, vb, M, d, *heads, beta1, beta2, one_minus_b1,
                     one_minus_b2, bc2_sqrt, eps);
  NV_CHECK_LAUNCH("nv_probe_step");
  return NV_OK;
}

extern "C" int nv_probe_predict(const float* Q, long ldq, int Nq, int d, const float* mean, const float* rstd, const float* W, const float* b, int H, int C,
                                float* logits, long ldl, float* probs, long ldp, void* stream) {
  NV_CHECK_ARG(H >= 1 && C >= 1 && H <= PMAXM && C <= PMAXM && H * C <= PMAXM, "nv_probe_predict: H=%d heads of C=%d columns: H * C must lie in [1, %d]", H, C, PMAXM);
  const int M = H * C;
  NV_CHECK_ARG(Q && W && b && logits && Nq > 0, "nv_probe_predict: null pointer or Nq=%d", Nq);
  NV_CHECK_ARG(d >= 4 && d <= NV_PROBE_MAX_D && (d % 4) == 0, "nv_probe_predict: d=%d must be a multiple of 4 in [4, %d]", d, NV_PROBE_MAX_D);
  NV_CHECK_ARG(ldq >= d && (ldq % 4) == 0 && nv_aligned16(Q) && nv_aligned16(W) && nv_aligned16(mean) && nv_aligned16(rstd),
               "nv_probe_predict: ldq=%ld must be a multiple of 4 with ldq >= d=%d; Q, W, mean and rstd 16-byte aligned", ldq, d);
  NV_CHECK_ARG((mean == nullptr) == (rstd == nullptr), "nv_probe_predict: mean and rstd are given together or not at all");
  NV_CHECK_ARG(ldl >= M && (!probs || ldp >= M), "nv_probe_predict: ldl=%ld and ldp=%ld must cover M=%d", ldl, ldp, M);
  NV_CHECK_ARG(nv_aligned(b, 4) && nv_aligned(logits, 4) && nv_aligned(probs, 4), "nv_probe_predict: b, logits and probs 4-byte aligned");
  ProbeArgs a{};
  a.X = Q; a.ldx = ldq; a.N = Nq; a.d = d; a.mean = mean; a.rstd = rstd; a.W = W; a.b = b;
  a.H = H; a.C = C; a.M = M; a.task = NV_PROBE_CLASSIFICATION;
  a.nchunks = probe_chunks(Nq);
  a.logits = logits; a.ldl = ldl; a.probs = probs; a.ldp = ldp;
  if (int rc = probe_launch<true>(a, a.nchunks, (hipStream_t)stream)) return rc;
  NV_CHECK_LAUNCH("nv_probe_predict");
  return NV_OK;
}
