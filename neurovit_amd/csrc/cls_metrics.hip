// Classification metrics on the device: the per-batch accumulation (nv_cls_metrics_update), the exact one-vs-rest ROC-AUC by pair counting
// (nv_cls_auc) and the finished table (nv_cls_metrics_finish); the labels of segments are in segments.hip.  The definitions are in the
// header.  Nothing here reads back, nothing uses atomics; every sum has one fixed order, so the bits reproduce from run to run.
#include <math.h>

#include "eval_common.h"

namespace {

constexpr int HEAD = NV_CLS_STATE_HEAD;

// ------------------------------------------------------------------------------------------------ update
// One workgroup.  The rows go by in chunks of 256, thread t taking row chunk + t: it forms the row's terms in double, keeps its own partial
// of nll and brier, and leaves a record (confusion cell, bin, conf, correct) in LDS.  Behind a barrier thread e owns the confusion cells e,
// e + 256, ... and thread b < bins the bin b: each walks the chunk's records in ascending row order and adds its find to the state - the
// owner of an address is always the same thread, so the read-modify-write needs no ordering beyond the stream's.
__global__ __launch_bounds__(256) void cls_update_kernel(const float* __restrict__ scores, long lds, const int* __restrict__ labels, int B, int C, int bins,
                                                         int kind, double* __restrict__ state, float* __restrict__ bank, long ldb,
                                                         int* __restrict__ bank_labels, long row0) {
  __shared__ int rcell[256], rbin[256], rhit[256];
  __shared__ double rconf[256];
  __shared__ double redd[4][4];
  const int tid = threadIdx.x;
  double acc_n = 0.0, acc_skip = 0.0, acc_nll = 0.0, acc_brier = 0.0;
  for (int chunk = 0; chunk < B; chunk += 256) {
    const int b = chunk + tid;
    int cell = -1, bin = 0, hit = 0;
    double conf = 0.0;
    if (b < B) {
      const float* z = scores + (long)b * lds;
      const int y = labels[b];
      bool ok = valid_label(y, C);
      float m = z[0];
      int pred = 0;
      for (int c = 0; c < C; ++c) {
        const float v = z[c];
        ok = ok && __builtin_isfinite(v);
        if (v > m) { m = v; pred = c; }      // strictly greater: the lowest index of the maximum
      }
      float* brow = bank ? bank + (row0 + b) * ldb : nullptr;
      if (bank_labels) bank_labels[row0 + b] = ok ? y : -1;
      if (!ok) {
        acc_skip += 1.0;
        if (brow)
          for (int c = 0; c < C; ++c) brow[c] = 0.f;
      } else {
        double S = 1.0, logS = 0.0;
        if (kind == NV_CLS_LOGITS) {
          S = 0.0;
          for (int c = 0; c < C; ++c) S += exp((double)z[c] - (double)m);
          logS = log(S);
        }
        double brier = 0.0, py = 0.0;
        for (int c = 0; c < C; ++c) {
          const double p = kind == NV_CLS_LOGITS ? exp((double)z[c] - (double)m) / S : (double)z[c];
          const double d = p - (c == y ? 1.0 : 0.0);
          brier += d * d;
          if (c == y) py = p;
          if (c == pred) conf = p;
          if (brow) brow[c] = (float)p;
        }
        const double nll = kind == NV_CLS_LOGITS ? ((double)m + logS) - (double)z[y] : -log(py);
        acc_n += 1.0; acc_nll += nll; acc_brier += brier;
        cell = y * C + pred;
        hit = pred == y;
        const double scaled = conf * (double)bins;
        bin = scaled >= (double)(bins - 1) ? bins - 1 : (scaled > 0.0 ? (int)scaled : 0);
      }
    }
    rcell[tid] = cell; rbin[tid] = bin; rhit[tid] = hit; rconf[tid] = conf;
    __syncthreads();
    const int rows = min(256, B - chunk);
    for (int e = tid; e < C * C; e += 256) {
      int cnt = 0;
      for (int r = 0; r < rows; ++r) cnt += rcell[r] == e;
      if (cnt) state[HEAD + e] += (double)cnt;
    }
    if (tid < bins) {
      int cnt = 0, hits = 0;
      double sc = 0.0;
      for (int r = 0; r < rows; ++r)
        if (rcell[r] >= 0 && rbin[r] == tid) { ++cnt; hits += rhit[r]; sc += rconf[r]; }
      if (cnt) {
        double* bs = state + HEAD + C * C;
        bs[tid] += (double)cnt; bs[bins + tid] += sc; bs[2 * bins + tid] += (double)hits;
      }
    }
    __syncthreads();      // the records are consumed before the next chunk overwrites them
  }
  double t[4] = {acc_n, acc_skip, acc_nll, acc_brier};
  block_sum4(t, redd);
  if (tid == 0) {
    state[0] += t[0]; state[1] += t[1]; state[2] += t[2]; state[5] += t[3];
    if (t[0] > 0.0) { state[3] += t[2] / t[0]; state[4] += 1.0; }
  }
}

// ------------------------------------------------------------------------------------------------ AUC
// Workgroup (x, y): thread t holds row i = 256 x + t, a positive of its own class c = y_i, and its probability p = probs[i][c].  The rows j of
// split y go through LDS in tiles of TJ rows, CLASS-major (tile[c][j], row pitch TJ + 4 floats, so a thread walks its own class with
// 16-byte reads and the classes of a 16-lane group fall on 16 different slots), beside the tile's labels.  An unusable row j is stored as
// NaN in every class and a thread without a usable label holds p = NaN: both compare false, so the inner loop has one predicate, y_j != c.
// TJ = min(256, 8192 / C rounded down to a multiple of 4): the tile is at most 8192 + 256 floats.
constexpr int AUC_TILE_FLOATS = 8192, AUC_TJ_MAX = 256, AUC_PAD = 4;
inline int auc_tile_rows(int C) {
  const int t = (AUC_TILE_FLOATS / C) & ~3;
  return t < AUC_TJ_MAX ? t : AUC_TJ_MAX;
}

__global__ __launch_bounds__(256) void cls_auc_kernel(const float* __restrict__ probs, long ldp, const int* __restrict__ labels, int N, int C, int TJ,
                                                      int tiles_per_split, int ntiles, int vec, unsigned long long* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) float tile[AUC_TILE_FLOATS + NV_CLS_MAX_C * AUC_PAD];
  __shared__ __attribute__((aligned(16))) int tlab[AUC_TJ_MAX];
  __shared__ int rc[256];
  __shared__ unsigned rgt[256], req[256];
  const int tid = threadIdx.x, pitch = TJ + AUC_PAD;
  const int i = blockIdx.x * 256 + tid;
  int c = 0;
  float p = __builtin_nanf("");
  bool active = false;
  if (i < N) {
    const int y = labels[i];
    if (valid_label(y, C)) { c = y; p = probs[(long)i * ldp + c]; active = true; }
  }
  unsigned gt = 0u, eq = 0u;
  const int t_begin = blockIdx.y * tiles_per_split, t_end = min(t_begin + tiles_per_split, ntiles);
  const float* mine = tile + c * pitch;
  for (int t = t_begin; t < t_end; ++t) {
    const int j0 = t * TJ, rows = min(TJ, N - j0);
    // labels first: every thread of the staging loop below reads its row's label from LDS
    for (int r = tid; r < TJ; r += 256) {
      int l = -1;
      if (r < rows) { l = labels[j0 + r]; if (!valid_label(l, C)) l = -1; }
      tlab[r] = l;
    }
    __syncthreads();
    const int cells = rows * C;
    if (vec) {      // ldp == C, 16-byte aligned base, j0 * C a multiple of 4: the tile's rows are one span of whole quads plus a tail
      const float* span = probs + (long)j0 * C;
      const int quads = cells >> 2;
      for (int q = tid; q < quads; q += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(span + 4 * q);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = 4 * q + u, r = e / C, cc = e - r * C;
          tile[cc * pitch + r] = tlab[r] < 0 ? __builtin_nanf("") : v[u];
        }
      }
      for (int e = 4 * quads + tid; e < cells; e += 256) {
        const int r = e / C, cc = e - r * C;
        tile[cc * pitch + r] = tlab[r] < 0 ? __builtin_nanf("") : span[e];
      }
    } else {
      for (int e = tid; e < cells; e += 256) {
        const int r = e / C, cc = e - r * C;
        tile[cc * pitch + r] = tlab[r] < 0 ? __builtin_nanf("") : probs[(long)(j0 + r) * ldp + cc];
      }
    }
    for (int e = cells + tid; e < TJ * C; e += 256) {      // rows past N (the last tile): unusable
      const int r = e / C, cc = e - r * C;
      tile[cc * pitch + r] = __builtin_nanf("");
    }
    __syncthreads();
    for (int r = 0; r < TJ; r += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(mine + r);
      const int4 l = *reinterpret_cast<const int4*>(tlab + r);
      gt += (unsigned)(l.x != c && p > v[0]) + (unsigned)(l.y != c && p > v[1]) + (unsigned)(l.z != c && p > v[2]) + (unsigned)(l.w != c && p > v[3]);
      eq += (unsigned)(l.x != c && p == v[0]) + (unsigned)(l.y != c && p == v[1]) + (unsigned)(l.z != c && p == v[2]) + (unsigned)(l.w != c && p == v[3]);
    }
    __syncthreads();      // the tile is consumed before the next one lands on it
  }
  rc[tid] = active ? c : -1; rgt[tid] = gt; req[tid] = eq;
  __syncthreads();
  if (tid < C) {
    unsigned long long g = 0ull, e = 0ull;
    for (int r = 0; r < 256; ++r)
      if (rc[r] == tid) { g += rgt[r]; e += req[r]; }
    unsigned long long* o = partial + (((long)blockIdx.y * gridDim.x + blockIdx.x) * C + tid) * 2;
    o[0] = g; o[1] = e;
  }
}

// One workgroup per class: thread t adds the partials of the workgroups t, t + 256, ... and counts the labels t, t + 256, ... - integers, so
// the order of the adds does not matter - then the wave butterfly and the four waves.
__global__ __launch_bounds__(256) void cls_auc_merge_kernel(const unsigned long long* __restrict__ partial, int groups, const int* __restrict__ labels, int N,
                                                            int C, double* __restrict__ out) {
  __shared__ unsigned long long red[4][4];
  const int c = blockIdx.x, tid = threadIdx.x;
  unsigned long long g = 0ull, e = 0ull, pos = 0ull, use = 0ull;
  for (int w = tid; w < groups; w += 256) {
    g += partial[((long)w * C + c) * 2];
    e += partial[((long)w * C + c) * 2 + 1];
  }
  for (int r = tid; r < N; r += 256) {
    const int l = labels[r];
    pos += l == c;
    use += valid_label(l, C);
  }
  unsigned long long t[4] = {g, e, pos, use};
  block_sum4(t, red);
  if (tid == 0) {
    const double gt = (double)t[0], eq = (double)t[1], n_pos = (double)t[2], n_neg = (double)(t[3] - t[2]);
    double* o = out + (long)c * NV_CLS_AUC_COLS;
    o[0] = (n_pos > 0.0 && n_neg > 0.0) ? (gt + 0.5 * eq) / (n_pos * n_neg) : (double)__builtin_nanf("");
    o[1] = n_pos; o[2] = n_neg; o[3] = gt; o[4] = eq;
  }
}

int auc_resolve_splits(int N, int C, int splits) {
  const int TJ = auc_tile_rows(C);
  return nv_resolve_splits((N + 255) / 256, (N + TJ - 1) / TJ, splits, NV_CLS_AUC_MAX_SPLITS);
}

bool auc_shape_ok(int N, int C, int splits) { return N >= 1 && N <= NV_CLS_AUC_MAX_N && C >= 2 && C <= NV_CLS_MAX_C && splits >= 0 && splits <= NV_CLS_AUC_MAX_SPLITS; }

// ------------------------------------------------------------------------------------------------ finish
// One workgroup, thread c = class c (C <= 64: one wave would do; the block is 64 threads).  The means over classes are formed by thread 0
// from LDS in ascending class order.
__global__ __launch_bounds__(64) void cls_finish_kernel(const double* __restrict__ state, int C, int bins, const double* __restrict__ auc, float* __restrict__ out) {
  __shared__ double srecall[NV_CLS_MAX_C], sf1[NV_CLS_MAX_C], sauc[NV_CLS_MAX_C], stp[NV_CLS_MAX_C];
  const int c = threadIdx.x;
  const double nan = (double)__builtin_nanf("");
  const double* conf = state + HEAD;
  if (c < C) {
    double support = 0.0, predicted = 0.0;
    for (int k = 0; k < C; ++k) { support += conf[c * C + k]; predicted += conf[k * C + c]; }
    const double tp = conf[c * C + c], den = support + predicted;      // 2TP + FP + FN
    const double recall = support > 0.0 ? tp / support : nan, precision = predicted > 0.0 ? tp / predicted : nan;
    const double f1 = den > 0.0 ? 2.0 * tp / den : nan, a = auc ? auc[(long)c * NV_CLS_AUC_COLS] : nan;
    srecall[c] = recall; sf1[c] = f1; sauc[c] = a; stp[c] = tp;
    float* o = out + NV_CLS_SCALARS + c * NV_CLS_CLASS_COLS;
    o[0] = (float)support; o[1] = (float)recall; o[2] = (float)precision; o[3] = (float)f1; o[4] = (float)a;
    float* cm = out + NV_CLS_SCALARS + C * NV_CLS_CLASS_COLS;
    for (int k = 0; k < C; ++k) cm[c * C + k] = (float)conf[c * C + k];
  }
  __syncthreads();
  if (c == 0) {
    const double n = state[0];
    double tp = 0.0, sr = 0.0, sf = 0.0, sa = 0.0;
    int nr = 0, nf = 0, na = 0;
    for (int k = 0; k < C; ++k) {
      tp += stp[k];
      if (srecall[k] == srecall[k]) { sr += srecall[k]; ++nr; }
      if (sf1[k] == sf1[k]) { sf += sf1[k]; ++nf; }
      if (sauc[k] == sauc[k]) { sa += sauc[k]; ++na; }
    }
    const double* bs = state + HEAD + C * C;
    double ece = 0.0;
    for (int b = 0; b < bins; ++b) ece += fabs(bs[2 * bins + b] - bs[bins + b]);
    const bool any = n > 0.0;
    out[0] = (float)n;
    out[1] = (float)state[1];
    out[2] = (float)(any ? tp / n : nan);
    out[3] = (float)((any && nr) ? sr / nr : nan);
    out[4] = (float)((any && nf) ? sf / nf : nan);
    out[5] = (float)(any ? state[2] / n : nan);
    out[6] = (float)(state[4] > 0.0 ? state[3] / state[4] : nan);
    out[7] = (float)(any ? state[5] / n : nan);
    out[8] = (float)(any ? ece / n : nan);
    out[9] = (float)(na ? sa / na : nan);
  }
}

}  // namespace

extern "C" long nv_cls_metrics_state_doubles(int C, int bins) {
  if (C < 2 || C > NV_CLS_MAX_C || bins < 1 || bins > NV_CLS_MAX_BINS) return 0;
  return (long)HEAD + (long)C * C + 3L * bins;
}

extern "C" long nv_cls_metrics_table_floats(int C) {
  if (C < 2 || C > NV_CLS_MAX_C) return 0;
  return (long)NV_CLS_SCALARS + (long)C * NV_CLS_CLASS_COLS + (long)C * C;
}

extern "C" int nv_cls_metrics_update(const float* scores, long lds, const int* labels, int B, int C, int bins, int kind, double* state, float* bank_probs,
                                     long ldb, int* bank_labels, long row0, long capacity, void* stream) {
  NV_CHECK_ARG(scores && labels && state && B >= 1, "nv_cls_metrics_update: null pointer or B=%d not positive", B);
  NV_CHECK_ARG(C >= 2 && C <= NV_CLS_MAX_C && bins >= 1 && bins <= NV_CLS_MAX_BINS, "nv_cls_metrics_update: C=%d outside [2, %d] or bins=%d outside [1, %d]", C,
               NV_CLS_MAX_C, bins, NV_CLS_MAX_BINS);
  NV_CHECK_ARG(kind == NV_CLS_LOGITS || kind == NV_CLS_PROBS, "nv_cls_metrics_update: unknown kind %d", kind);
  NV_CHECK_ARG(lds >= C, "nv_cls_metrics_update: lds=%ld must cover C=%d", lds, C);
  NV_CHECK_ARG(nv_aligned(state, 8) && nv_aligned(scores, 4) && nv_aligned(labels, 4), "nv_cls_metrics_update: state 8-byte aligned, scores and labels 4-byte aligned");
  NV_CHECK_ARG((bank_probs == nullptr) == (bank_labels == nullptr), "nv_cls_metrics_update: bank_probs and bank_labels are given together or not at all");
  if (bank_probs) {
    NV_CHECK_ARG(ldb >= C && nv_aligned(bank_probs, 4) && nv_aligned(bank_labels, 4), "nv_cls_metrics_update: ldb=%ld must cover C=%d; the bank 4-byte aligned", ldb, C);
    NV_CHECK_ARG(row0 >= 0 && capacity >= 0 && row0 <= capacity && (long)B <= capacity - row0, "nv_cls_metrics_update: %d rows from row0=%ld do not fit a bank of %ld rows", B,
                 row0, capacity);
  }
  hipLaunchKernelGGL(cls_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scores, lds, labels, B, C, bins, kind, state, bank_probs, ldb, bank_labels, row0);
  NV_CHECK_LAUNCH("nv_cls_metrics_update");
  return NV_OK;
}

extern "C" int nv_cls_auc_splits(int N, int C, int splits) { return auc_shape_ok(N, C, splits) ? auc_resolve_splits(N, C, splits) : 0; }

extern "C" long nv_cls_auc_workspace_bytes(int N, int C, int splits) {
  const int s = nv_cls_auc_splits(N, C, splits);
  if (s < 1) return 0;
  return (long)s * ((N + 255) / 256) * C * 2L * (long)sizeof(unsigned long long);
}

extern "C" int nv_cls_auc(const float* probs, long ldp, const int* labels, int N, int C, int splits, double* out, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(probs && labels && out && workspace, "nv_cls_auc: null pointer");
  NV_CHECK_ARG(N >= 1 && N <= NV_CLS_AUC_MAX_N, "nv_cls_auc: N=%d outside [1, %d] (the 32-bit counts of a thread and the exact doubles of the totals)", N, NV_CLS_AUC_MAX_N);
  NV_CHECK_ARG(C >= 2 && C <= NV_CLS_MAX_C, "nv_cls_auc: C=%d outside [2, %d]", C, NV_CLS_MAX_C);
  NV_CHECK_ARG(splits >= 0 && splits <= NV_CLS_AUC_MAX_SPLITS, "nv_cls_auc: splits=%d outside [0, %d] (0 = automatic)", splits, NV_CLS_AUC_MAX_SPLITS);
  NV_CHECK_ARG(ldp >= C, "nv_cls_auc: ldp=%ld must cover C=%d", ldp, C);
  NV_CHECK_ARG(nv_aligned(probs, 4) && nv_aligned(labels, 4) && nv_aligned(out, 8) && nv_aligned(workspace, 8), "nv_cls_auc: probs and labels 4-byte, out and workspace 8-byte aligned");
  const int S = auc_resolve_splits(N, C, splits);
  const long need = nv_cls_auc_workspace_bytes(N, C, S);
  NV_CHECK_ARG(ws_bytes >= need, "nv_cls_auc: %d splits need a workspace of %ld bytes (nv_cls_auc_workspace_bytes), got %ld", S, need, ws_bytes);
  const int TJ = auc_tile_rows(C), itiles = (N + 255) / 256, jtiles = (N + TJ - 1) / TJ, tps = (jtiles + S - 1) / S;
  static_assert(((AUC_TILE_FLOATS / NV_CLS_MAX_C) & ~3) >= 4, "a tile holds at least four rows of the widest bank");
  static_assert(NV_CLS_AUC_MAX_N < (1L << 31) && NV_CLS_AUC_MAX_SPLITS <= 65535, "32-bit thread counts; the grid's y extent");
  const int vec = (ldp == C && nv_aligned16(probs)) ? 1 : 0;      // (j0 * C is a multiple of 4: TJ is)
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* partial = (unsigned long long*)workspace;
  hipLaunchKernelGGL(cls_auc_kernel, dim3(itiles, S), dim3(256), 0, s, probs, ldp, labels, N, C, TJ, tps, jtiles, vec, partial);
  hipLaunchKernelGGL(cls_auc_merge_kernel, dim3(C), dim3(256), 0, s, partial, itiles * S, labels, N, C, out);
  NV_CHECK_LAUNCH("nv_cls_auc");
  return NV_OK;
}

extern "C" int nv_cls_metrics_finish(const double* state, int C, int bins, const double* auc, float* out, void* stream) {
  NV_CHECK_ARG(state && out, "nv_cls_metrics_finish: null pointer");
  NV_CHECK_ARG(C >= 2 && C <= NV_CLS_MAX_C && bins >= 1 && bins <= NV_CLS_MAX_BINS, "nv_cls_metrics_finish: C=%d outside [2, %d] or bins=%d outside [1, %d]", C, NV_CLS_MAX_C,
               bins, NV_CLS_MAX_BINS);
  NV_CHECK_ARG(nv_aligned(state, 8) && nv_aligned(auc, 8) && nv_aligned(out, 4), "nv_cls_metrics_finish: state and auc 8-byte, out 4-byte aligned");
  hipLaunchKernelGGL(cls_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, C, bins, auc, out);
  NV_CHECK_LAUNCH("nv_cls_metrics_finish");
  return NV_OK;
}
