// Attribution for the 4D model: the steps that see a SERIES of T volumes per sample, where attribution.hip sees one volume.
//
//   nv_gradcam_reduce_grouped   the Grad-CAM reduction with the min-max taken over `group` consecutive volumes (a sample's T timepoints)
//   nv_series_map_to_volumes    maps [B, T, N] -> normalisation and percentile cut over the sample's T N cells jointly (scope SERIES) or per
//                               volume (scope VOLUME) -> trilinear upsampling into [B, S0, S1, S2, T] (layout SERIES: time innermost, the
//                               layout of the model's input and of a 4D NIfTI) or [B, T, S0, S1, S2] (layout FRAMES)
//   nv_series_leave_one_out     z [B, T, 2] + z_base [2] -> the B (T + 1) sequences of temporal occlusion
//   nv_temporal_grad_x_input    sum_c dx[b, t, c] z[b, t, c]
//
// The reduction, the selection and the frames-layout upsampling are attribution.hip's kernels (attr_common.h declares their launchers
// and holds the device code both files run); new here are the selection over a whole series in one workgroup's LDS and the upsampling
// that writes time innermost in one pass.
#include "attr_common.h"

namespace {
constexpr int SS_THREADS = 1024;         // selection over a series: one workgroup per sample
constexpr int SS_MAX_T = 64;             // the temporal head's limit (temporal.hip: TH_MAXT)
constexpr int SS_MAX_CELLS = 32768;      // T N cells of one sample: 128 KiB of keys in LDS
constexpr int TM_MAX_CELLS = 4096;       // cells of one volume (scope VOLUME: attribution.hip's kernel)
constexpr int SU_THREADS = 256;
constexpr long SU_MAX_LDS_FLOATS = 40960;        // 160 KiB: G1 G2 T + 2 S1 + 2 S2 floats of one workgroup

// One workgroup per sample: threshold_block over the sample's T N cells, keys in dynamic LDS.
__global__ __launch_bounds__(SS_THREADS) void series_threshold_kernel(const float* __restrict__ maps, int TN, int normalize, QuantilePos pos,
                                                                      float* __restrict__ norm, float* __restrict__ sparse, float* __restrict__ cuts) {
  extern __shared__ unsigned series_keys[];
  __shared__ ThresholdScratch scratch;
  const long off = (long)blockIdx.x * TN;
  const float cut = threshold_block<SS_THREADS>(maps + off, TN, normalize, pos, norm + off, sparse + off, series_keys, scratch);
  if (threadIdx.x == 0) cuts[blockIdx.x] = cut;
}

// Grid (S0, B): one workgroup writes the output plane (b, x) of layout SERIES, S1 * S2 * T contiguous floats.  It collapses the x axis of
// the sample's T grids into an LDS plane [G1][G2][T] (t fastest: the lanes of a wave walk t, then z, and hit consecutive banks) and
// tabulates the y and z taps; every output then costs four LDS reads and three lerps - upsample_trilinear_kernel's operations in its
// order (blend, plane_value), so out[b, x, y, z, t] has the bits of that kernel's out[b * T + t, x, y, z].  16-byte stores over the flat
// extent (split_span: S2 * T need not be a multiple of four).
__global__ __launch_bounds__(SU_THREADS) void upsample_series_kernel(const float* __restrict__ sparse, int T, int G0, int G1, int G2, int S0, int S1, int S2,
                                                                     float sc0, float sc1, float sc2, float* __restrict__ out) {
  extern __shared__ float smem[];
  const int cells = G1 * G2;
  float* plane = smem;                                     // [G1 * G2][T]
  int* yi = reinterpret_cast<int*>(plane + cells * T);     // [S1]: i0 | i1 << 16
  float* yl = reinterpret_cast<float*>(yi + S1);           // [S1]: lambda1
  int* zi = reinterpret_cast<int*>(yl + S1);               // [S2]
  float* zl = reinterpret_cast<float*>(zi + S2);           // [S2]
  const int tid = threadIdx.x, x = blockIdx.x, b = blockIdx.y;
  const AxisTap tx = axis_tap(x, sc0, G0);
  const long N = (long)G0 * cells;
  const float* g0 = sparse + (long)b * T * N + (long)tx.i0 * cells;       // grid t: + t N
  const float* g1 = sparse + (long)b * T * N + (long)tx.i1 * cells;
  for (int i = tid; i < cells * T; i += SU_THREADS) {      // (read in the order the grids lie, written t-fastest)
    const int t = i / cells, rc = i - t * cells;
    plane[rc * T + t] = blend(tx.l0, g0[t * N + rc], tx.l1, g1[t * N + rc]);
  }
  fill_axis_table(yi, yl, S1, sc1, G1, G2, tid, SU_THREADS);
  fill_axis_table(zi, zl, S2, sc2, G2, 1, tid, SU_THREADS);
  __syncthreads();

  const int row = S2 * T;                                  // floats of one output row y
  const long plane_elems = (long)S1 * row;
  const long base = ((long)b * S0 + x) * plane_elems;      // flat offset of the plane in `out`
  float* o = out + base;
  const int P = (int)plane_elems;
  const Span s = split_span(base, P);                      // `out` is 16-byte aligned

  auto single = [&](int e) {
    const int y = e / row, r = e - y * row, z = r / T, t = r - z * T;
    o[e] = plane_value(plane + t, T, yi[y], yl[y], zi[z], zl[z]);
  };
  for (int e = tid; e < s.head; e += SU_THREADS) single(e);
  for (int e = s.tail + tid; e < P; e += SU_THREADS) single(e);
  for (int g = tid; g < s.groups; g += SU_THREADS) {
    const int e = s.head + 4 * g;
    int y = e / row, r = e - y * row, z = r / T, t = r - z * T;
    int yy = yi[y], zz = zi[z];
    float ly1 = yl[y], lz1 = zl[z];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = plane_value(plane + t, T, yy, ly1, zz, lz1);
      if (j < 3 && ++t == T) {                             // (a group may straddle cells and rows; y < S1 because e + j < P)
        t = 0;
        if (++z == S2) { z = 0; ++y; yy = yi[y]; ly1 = yl[y]; }
        zz = zi[z]; lz1 = zl[z];
      }
    }
    *reinterpret_cast<f32x4*>(o + e) = v;
  }
}

constexpr int EW_THREADS = 256;

// out [B (T + 1), T, 2]: row b (T + 1) is z[b]; row b (T + 1) + 1 + k is z[b] with timepoint k replaced by z_base.  A pure select.
__global__ __launch_bounds__(EW_THREADS) void leave_one_out_kernel(const float* __restrict__ z, const float* __restrict__ z_base, int T, long total,
                                                                   float* __restrict__ out) {
  const long i = (long)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i & 1);
  const long q = i >> 1;                                   // (row, t)
  const int t = (int)(q % T);
  const long r = q / T;
  const int k = (int)(r % (T + 1));
  const long b = r / (T + 1);
  out[i] = (k == t + 1) ? z_base[c] : z[(b * T + t) * 2 + c];
}

// out[b, t] = dx[b, t, 0] z[b, t, 0] + dx[b, t, 1] z[b, t, 1]: two products and one sum, each rounded on its own (no FMA)
__global__ __launch_bounds__(EW_THREADS) void grad_x_input_kernel(const float* __restrict__ dx, const float* __restrict__ z, long rows, float* __restrict__ out) {
#pragma clang fp contract(off)
  const long i = (long)blockIdx.x * EW_THREADS + threadIdx.x;
  if (i >= rows) return;
  const float p0 = dx[2 * i] * z[2 * i];
  const float p1 = dx[2 * i + 1] * z[2 * i + 1];
  out[i] = p0 + p1;
}

bool grid_ok(const int* g) { return g && g[0] > 0 && g[1] > 0 && g[2] > 0; }
bool scope_ok(int scope) { return scope == NV_SERIES_SCOPE_SERIES || scope == NV_SERIES_SCOPE_VOLUME; }
}  // namespace

extern "C" long nv_gradcam_grouped_workspace_bytes(int V, int n, int group) {
  if (V <= 0 || n <= 1 || group <= 0 || V % group != 0) return -1;
  const int groups = V / group;
  return nv_attr_gc_workspace_bytes(groups, nv_attr_gc_blocks((long)group * (n - 1), groups));
}

extern "C" int nv_gradcam_reduce_grouped(const void* act, const float* grad, int V, int n, int d, int group, float* cam, float* minmax, void* workspace,
                                         long ws_bytes, void* stream) {
  NV_CHECK_ARG(act && grad && cam && workspace && V > 0 && n > 1 && d > 0 && (d % 8) == 0, "nv_gradcam_reduce_grouped: bad arguments (d %% 8 == 0, n > 1)");
  NV_CHECK_ARG(group > 0 && V % group == 0 && V / group <= 65535, "nv_gradcam_reduce_grouped: %d volumes are no whole number (<= 65535) of groups of %d", V, group);
  NV_CHECK_ARG((long)V * (n - 1) < (1L << 31), "nv_gradcam_reduce_grouped: %d volumes of %d tokens beyond one launch", V, n - 1);
  NV_CHECK_ARG(nv_aligned16(act) && nv_aligned16(grad) && nv_aligned16(workspace) && nv_aligned(cam, 4) && nv_aligned(minmax, 4),
               "nv_gradcam_reduce_grouped: 16-byte alignment");
  NV_CHECK_ARG(ws_bytes >= nv_gradcam_grouped_workspace_bytes(V, n, group), "nv_gradcam_reduce_grouped: workspace too small");
  const int groups = V / group, R = group * (n - 1);
  return nv_attr_gradcam_launch("nv_gradcam_reduce_grouped", act, grad, n, d, groups, R, nv_attr_gc_blocks(R, groups), cam, minmax, workspace, stream);
}

extern "C" long nv_series_map_to_volumes_workspace_bytes(int B, int T, const int* grid3, int scope) {
  if (B <= 0 || T <= 0 || T > SS_MAX_T || !grid_ok(grid3) || !scope_ok(scope)) return -1;
  const long N = (long)grid3[0] * grid3[1] * grid3[2];
  return (2 * (long)B * T * N + (scope == NV_SERIES_SCOPE_SERIES ? B : (long)B * T)) * 4;
}

extern "C" int nv_series_map_to_volumes(const float* maps, int B, int T, const int* grid3, const int* out3, int normalize, int scope, double keep_percent,
                                        int layout, float* out, void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(maps && grid3 && out3 && out && workspace && B > 0 && B <= 65535, "nv_series_map_to_volumes: bad arguments (null pointer, or B outside [1, 65535])");
  NV_CHECK_ARG(T >= 1 && T <= SS_MAX_T, "nv_series_map_to_volumes: %d timepoints outside [1, %d]", T, SS_MAX_T);
  NV_CHECK_ARG(scope_ok(scope) && (layout == NV_SERIES_LAYOUT_SERIES || layout == NV_SERIES_LAYOUT_FRAMES),
               "nv_series_map_to_volumes: scope %d / layout %d is none of the NV_SERIES_* constants", scope, layout);
  const int G0 = grid3[0], G1 = grid3[1], G2 = grid3[2], S0 = out3[0], S1 = out3[1], S2 = out3[2];
  NV_CHECK_ARG(G0 > 0 && G1 > 0 && G2 > 0 && S0 > 0 && S1 > 0 && S2 > 0, "nv_series_map_to_volumes: grid and output extents must be positive");
  const long N = (long)G0 * G1 * G2, TN = (long)T * N, V = (long)B * T;
  NV_CHECK_ARG(N <= TM_MAX_CELLS, "nv_series_map_to_volumes: grid %d x %d x %d has %ld cells, the kernels take at most %d (16^3)", G0, G1, G2, N, TM_MAX_CELLS);
  if (scope == NV_SERIES_SCOPE_SERIES) {
    NV_CHECK_ARG(TN <= SS_MAX_CELLS, "nv_series_map_to_volumes: %d timepoints of %ld cells are %ld cells per sample, scope SERIES takes at most %d - use scope VOLUME",
                 T, N, TN, SS_MAX_CELLS);
  }
  NV_CHECK_ARG(keep_percent >= 0.0 && keep_percent <= 100.0, "nv_series_map_to_volumes: keep_percent %g outside [0, 100]", keep_percent);
  const long lds_frames = (long)G1 * G2 + 2L * S1 + 2L * S2, lds_series = (long)G1 * G2 * T + 2L * S1 + 2L * S2;
  if (layout == NV_SERIES_LAYOUT_SERIES) {
    NV_CHECK_ARG(lds_series <= SU_MAX_LDS_FLOATS && (long)S1 * S2 * T < (1L << 31),
                 "nv_series_map_to_volumes: output extents %d x %d x %d x %d beyond the kernel's tables (G1 G2 T + 2 S1 + 2 S2 <= %ld)", S0, S1, S2, T, SU_MAX_LDS_FLOATS);
  } else {
    NV_CHECK_ARG(lds_frames <= 16384 && (long)S1 * S2 < (1L << 31) && V <= 65535,
                 "nv_series_map_to_volumes: output extents %d x %d x %d beyond the kernel's tables (G1 G2 + 2 S1 + 2 S2 <= 16384), or B T > 65535", S0, S1, S2);
  }
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned16(workspace) && nv_aligned(maps, 4), "nv_series_map_to_volumes: out / workspace 16-byte aligned");
  NV_CHECK_ARG(ws_bytes >= nv_series_map_to_volumes_workspace_bytes(B, T, grid3, scope), "nv_series_map_to_volumes: workspace too small");
  float* norm = (float*)workspace;
  float* sparse = norm + V * N;
  float* cuts = sparse + V * N;
  hipStream_t s = (hipStream_t)stream;
  if (scope == NV_SERIES_SCOPE_SERIES) {
    static bool allowed = false;
    const int rc = allow_lds(series_threshold_kernel, SS_MAX_CELLS * 4, allowed, "nv_series_map_to_volumes (threshold)");
    if (rc != NV_OK) return rc;
    hipLaunchKernelGGL(series_threshold_kernel, dim3(B), dim3(SS_THREADS), (size_t)TN * 4, s, maps, (int)TN, normalize ? 1 : 0, quantile_pos(keep_percent, TN), norm,
                       sparse, cuts);
    NV_CHECK_LAUNCH("nv_series_map_to_volumes (threshold)");
  } else {
    const int rc = nv_attr_threshold_launch("nv_series_map_to_volumes (threshold)", maps, (int)V, (int)N, normalize, keep_percent, norm, sparse, cuts, stream);
    if (rc != NV_OK) return rc;
  }
  if (layout == NV_SERIES_LAYOUT_FRAMES) return nv_attr_upsample_launch("nv_series_map_to_volumes (upsample)", sparse, (int)V, grid3, out3, out, stream);
  static bool allowed = false;
  const int rc = allow_lds(upsample_series_kernel, (int)(SU_MAX_LDS_FLOATS * 4), allowed, "nv_series_map_to_volumes (upsample)");
  if (rc != NV_OK) return rc;
  hipLaunchKernelGGL(upsample_series_kernel, dim3(S0, B), dim3(SU_THREADS), (size_t)lds_series * 4, s, sparse, T, G0, G1, G2, S0, S1, S2, (float)G0 / (float)S0,
                     (float)G1 / (float)S1, (float)G2 / (float)S2, out);
  NV_CHECK_LAUNCH("nv_series_map_to_volumes (upsample)");
  return NV_OK;
}

extern "C" int nv_series_leave_one_out(const float* z, const float* z_base, int B, int T, float* out, void* stream) {
  NV_CHECK_ARG(z && z_base && out && B > 0 && T >= 1 && T <= SS_MAX_T, "nv_series_leave_one_out: bad arguments (null pointer, B not positive, or T outside [1, %d])",
               SS_MAX_T);
  NV_CHECK_ARG(nv_aligned(z, 4) && nv_aligned(z_base, 4) && nv_aligned(out, 4), "nv_series_leave_one_out: element-aligned buffers");
  const long total = (long)B * (T + 1) * T * 2, blocks = (total + EW_THREADS - 1) / EW_THREADS;
  NV_CHECK_ARG(blocks < (1L << 31), "nv_series_leave_one_out: %d samples beyond one launch", B);
  hipLaunchKernelGGL(leave_one_out_kernel, dim3((unsigned)blocks), dim3(EW_THREADS), 0, (hipStream_t)stream, z, z_base, T, total, out);
  NV_CHECK_LAUNCH("nv_series_leave_one_out");
  return NV_OK;
}

extern "C" int nv_temporal_grad_x_input(const float* dx, const float* z, int B, int T, float* out, void* stream) {
  NV_CHECK_ARG(dx && z && out && B > 0 && T >= 1 && T <= SS_MAX_T, "nv_temporal_grad_x_input: bad arguments (null pointer, B not positive, or T outside [1, %d])",
               SS_MAX_T);
  NV_CHECK_ARG(nv_aligned(dx, 4) && nv_aligned(z, 4) && nv_aligned(out, 4), "nv_temporal_grad_x_input: element-aligned buffers");
  const long rows = (long)B * T, blocks = (rows + EW_THREADS - 1) / EW_THREADS;
  hipLaunchKernelGGL(grad_x_input_kernel, dim3((unsigned)blocks), dim3(EW_THREADS), 0, (hipStream_t)stream, dx, z, rows, out);
  NV_CHECK_LAUNCH("nv_temporal_grad_x_input");
  return NV_OK;
}
