// Batched, device-side attribution volumes: [B, n, d] taps or [B, N] token maps in, [B, S0, S1, S2] volumes out - the last step of
// get_attention_map / get_attention_rollout / get_attention_relevance (src/models/NeuroEncoder.py:101-131) for a whole batch, every
// volume on its own.
//
//   nv_gradcam_reduce              the Grad-CAM reduction of get_attention_map, min-max normalised over the whole [B, n-1] map
//   nv_gradcam_reduce_per_volume   the same row arithmetic, min-max normalised over each volume's own cells
//   nv_token_map_to_volume         per volume: min-max normalisation (optional) -> the percentile cut of torch.quantile(linear) ->
//                                  threshold -> trilinear upsampling (align_corners = False, ATen's index arithmetic)
//
// The only real bytes are the B * S0 * S1 * S2 * 4 of the volumes: the upsampling is a streaming kernel with 16-byte stores along the
// contiguous axis; everything in front of it works on <= 4096 cells per volume inside one workgroup's LDS.
#include "attr_common.h"

namespace {
// ------------------------------------------------------------------------------------------------ Grad-CAM reduction
// The reduction of the reference's NeuroEncoder.get_attention_map (src/models/NeuroEncoder.py:101-116) as ONE launch.
//
//   weights[b,t] = mean_d grad[b,t,:]          cam[b,t] = sum_d weights[b,t] * act[b,t,:] = weights[b,t] * sum_d act[b,t,:]
//   cam = relu(cam[:, 1:])  (cls token dropped)  ->  (cam - min) / (max - min + 1e-8)  over a group of cells
//
// act = output of the last block's attention LayerNorm (16-bit, the engine's xn1 buffer), grad = its gradient (fp32, the engine's
// hookg buffer): 2 x [B, n, d] on the device -> [B, n-1] floats.  HBM-bound (reads 6 B per element once).
constexpr int GC_THREADS = 256;
constexpr int GC_WAVES = GC_THREADS / 64;
constexpr int GC_MAX_BLOCKS = 512;       // workgroups of the whole map (nv_gradcam_reduce)
constexpr int GCV_MAX_BLOCKS = 128;      // workgroups per volume (nv_gradcam_reduce_per_volume)

// Grid (blocks per group, groups).  A group is `R` consecutive rows of the flat [B * (n-1)] map that share one min / max: the whole map
// (one group of B (n-1) rows) or one volume (B groups of n-1 rows).  Flat row r is token r % N + 1 of volume r / N (token 0 is the cls
// token).  One wave per row (two row reductions by wave shuffles); the rows of a group are dealt over its blocks, its min / max
// crosses them through per-block partials and ONE arrival ticket per group: the LAST block of a group to arrive normalises that
// group's (tiny) map.  The hand-off is the placement-independent agent-scope release / acquire of the CDNA4 guide (Guideline 16):
// results do not depend on which workgroup is last, and min / max are exact in any order, so a volume has the same bits whether it
// is reduced alone, as one group of a batch, or as part of a whole-batch group with the same extremes.
template <typename T>
__global__ __launch_bounds__(GC_THREADS) void gradcam_reduce_kernel(const r16* __restrict__ act, const float* __restrict__ grad, int n, int d, int R,
                                                                    float* cam, float* __restrict__ part, unsigned* tickets, float* minmax) {
  __shared__ float s_min[GC_WAVES], s_max[GC_WAVES];
  __shared__ unsigned s_last;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int N = n - 1, g = blockIdx.y, nb = gridDim.x;
  const int b0 = g * (R / N), t0 = g * (R % N);          // the group's first flat row g R = b0 N + t0, in 32-bit arithmetic (t0 may pass N)
  float* gcam = cam + (long)g * R;
  float* gpart = part + 2L * g * nb;
  float lo = INFINITY, hi = 0.f;                         // relu output is >= 0, every workgroup owns >= 0 rows
  for (int i = blockIdx.x * GC_WAVES + wid; i < R; i += nb * GC_WAVES) {
    const int q = t0 + i, b = b0 + q / N, t = q - (q / N) * N + 1;
    const long base = ((long)b * n + t) * d;
    float sg = 0.f, sa = 0.f;
    for (int k = lane * 8; k < d; k += 64 * 8) {         // d % 8 == 0 (engine requirement)
      const r16x8 a = *reinterpret_cast<const r16x8*>(act + base + k);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(grad + base + k), g1 = *reinterpret_cast<const f32x4*>(grad + base + k + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) sa += dec1<T>(a[j]);
      sg += (g0[0] + g0[1]) + (g0[2] + g0[3]) + (g1[0] + g1[1]) + (g1[2] + g1[3]);
    }
    sg = wave_sum(sg); sa = wave_sum(sa);
    const float v = fmaxf((sg / (float)d) * sa, 0.f);
    if (lane == 0) gcam[i] = v;
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  if (lane == 0) { s_min[wid] = lo; s_max[wid] = hi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < GC_WAVES; ++w) { lo = fminf(lo, s_min[w]); hi = fmaxf(hi, s_max[w]); }
    gpart[2 * blockIdx.x] = lo; gpart[2 * blockIdx.x + 1] = hi;
  }
  // publish: every storing wave drains its stores, the workgroup meets, ONE lane releases at agent scope and takes a ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned tk = __hip_atomic_fetch_add(tickets + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (tk == (unsigned)nb - 1) ? 1u : 0u;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  if (!s_last) return;
  // last arriver of this group: min / max of its partials (fixed order), then normalise its map
  lo = INFINITY; hi = 0.f;
  for (int i = 0; i < nb; ++i) { lo = fminf(lo, gpart[2 * i]); hi = fmaxf(hi, gpart[2 * i + 1]); }
  const float inv = 1.0f / (hi - lo + 1e-8f);
  for (int i = tid; i < R; i += GC_THREADS) gcam[i] = (gcam[i] - lo) * inv;
  if (tid == 0) {
    if (minmax) { minmax[2 * g] = lo; minmax[2 * g + 1] = hi; }
    tickets[g] = 0;                                       // self-reset (the caller also zeroes the tickets in front of every launch)
  }
}

// ------------------------------------------------------------------------------------------------ token maps -> thresholded maps
constexpr int TM_THREADS = 256;
constexpr int TM_MAX_CELLS = 4096;       // cells of one volume's grid: 16 KB of keys in LDS (16^3 = ViT3D-large)

// One workgroup per volume.  norm / sparse: [B, N] (the normalised map, and the same with the cells under the cut zeroed); cuts: [B].
// pos: the position q (N - 1) of the quantile among the order statistics (quantile_pos); the work is threshold_block's.
__global__ __launch_bounds__(TM_THREADS) void token_map_threshold_kernel(const float* __restrict__ maps, int N, int normalize, QuantilePos pos,
                                                                         float* __restrict__ norm, float* __restrict__ sparse, float* __restrict__ cuts) {
  __shared__ unsigned keys[TM_MAX_CELLS];
  __shared__ ThresholdScratch scratch;
  const long off = (long)blockIdx.x * N;
  const float cut = threshold_block<TM_THREADS>(maps + off, N, normalize, pos, norm + off, sparse + off, keys, scratch);
  if (threadIdx.x == 0) cuts[blockIdx.x] = cut;
}

// ------------------------------------------------------------------------------------------------ trilinear upsampling
constexpr int UP_THREADS = 256;
// Grid (S0, B): one workgroup writes the S1 x S2 output plane (b, x).  It first collapses the x axis of the volume's grid into a
// G1 x G2 plane in LDS and tabulates the y and z taps; every output then costs four LDS reads and three lerps.  The plane is written as
// 16-byte stores over its flat extent (rows need not be multiples of four: split_span, the groups of four follow the alignment of `out`).
__global__ __launch_bounds__(UP_THREADS) void upsample_trilinear_kernel(const float* __restrict__ sparse, int G0, int G1, int G2, int S0, int S1, int S2,
                                                                        float sc0, float sc1, float sc2, float* __restrict__ out) {
  extern __shared__ float smem[];
  float* plane = smem;                                     // [G1 * G2]
  int* yi = reinterpret_cast<int*>(plane + G1 * G2);       // [S1]: i0 | i1 << 16
  float* yl = reinterpret_cast<float*>(yi + S1);           // [S1]: lambda1
  int* zi = reinterpret_cast<int*>(yl + S1);               // [S2]
  float* zl = reinterpret_cast<float*>(zi + S2);           // [S2]
  const int tid = threadIdx.x, x = blockIdx.x, b = blockIdx.y;
  const AxisTap tx = axis_tap(x, sc0, G0);
  const float* g0 = sparse + ((long)b * G0 + tx.i0) * G1 * G2;
  const float* g1 = sparse + ((long)b * G0 + tx.i1) * G1 * G2;
  for (int i = tid; i < G1 * G2; i += UP_THREADS) plane[i] = blend(tx.l0, g0[i], tx.l1, g1[i]);
  fill_axis_table(yi, yl, S1, sc1, G1, G2, tid, UP_THREADS);
  fill_axis_table(zi, zl, S2, sc2, G2, 1, tid, UP_THREADS);
  __syncthreads();

  const long plane_elems = (long)S1 * S2;
  const long base = ((long)b * S0 + x) * plane_elems;      // flat offset of the plane in `out`
  float* o = out + base;
  const int P = (int)plane_elems;
  const Span s = split_span(base, P);                      // `out` is 16-byte aligned

  // (yy, ly1): the y taps of the row, read once per row
  auto value = [&](int yy, float ly1, int z) -> float { return plane_value(plane, 1, yy, ly1, zi[z], zl[z]); };
  for (int e = tid; e < s.head; e += UP_THREADS) { const int y = e / S2; o[e] = value(yi[y], yl[y], e - y * S2); }
  for (int e = s.tail + tid; e < P; e += UP_THREADS) { const int y = e / S2; o[e] = value(yi[y], yl[y], e - y * S2); }
  for (int g = tid; g < s.groups; g += UP_THREADS) {
    const int e = s.head + 4 * g;
    int y = e / S2, z = e - y * S2;
    int yy = yi[y];
    float ly1 = yl[y];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = value(yy, ly1, z);
      if (++z == S2 && j < 3) { z = 0; ++y; yy = yi[y]; ly1 = yl[y]; }     // (a group may straddle rows; y < S1 because e + j < P)
    }
    *reinterpret_cast<f32x4*>(o + e) = v;
  }
}

int gc_blocks(long rows, int cap) {
  const long blocks = (rows + GC_WAVES - 1) / GC_WAVES;
  return blocks > cap ? cap : (blocks < 1 ? 1 : (int)blocks);
}
long gc_ticket_bytes(int groups) { return ((4L * groups + 15) / 16) * 16; }

}  // namespace

// workspace: the groups' tickets (zeroed here), then 2 floats per block and group
int nv_attr_gradcam_launch(const char* name, const void* act, const float* grad, int n, int d, int groups, int R, int blocks, float* cam, float* minmax,
                           void* workspace, void* stream) {
  unsigned* tickets = (unsigned*)workspace;
  float* part = (float*)((char*)workspace + gc_ticket_bytes(groups));
  if (hipMemsetAsync(tickets, 0, gc_ticket_bytes(groups), (hipStream_t)stream) != hipSuccess) {
    nv_set_error("%s: memset failed", name);
    return NV_ERR_HIP;
  }
  NV_DISPATCH_OPERAND(T, hipLaunchKernelGGL(gradcam_reduce_kernel<T>, dim3(blocks, groups), dim3(GC_THREADS), 0, (hipStream_t)stream, (const r16*)act, grad, n,
                                            d, R, cam, part, tickets, minmax));
  NV_CHECK_LAUNCH(name);
  return NV_OK;
}

extern "C" long nv_gradcam_workspace_bytes(int B, int n) { return gc_ticket_bytes(1) + 8L * gc_blocks((long)B * (n - 1), GC_MAX_BLOCKS); }

extern "C" int nv_gradcam_reduce(const void* act, const float* grad, int B, int n, int d, float* cam, float* minmax, void* workspace,
                                 long ws_bytes, void* stream) {
  NV_CHECK_ARG(act && grad && cam && workspace && B > 0 && n > 1 && d > 0 && (d % 8) == 0, "nv_gradcam_reduce: bad arguments (d %% 8 == 0, n > 1)");
  NV_CHECK_ARG(nv_aligned16(act) && nv_aligned16(grad) && nv_aligned16(workspace), "nv_gradcam_reduce: 16-byte alignment");
  NV_CHECK_ARG(ws_bytes >= nv_gradcam_workspace_bytes(B, n), "nv_gradcam_reduce: workspace too small");
  return nv_attr_gradcam_launch("nv_gradcam_reduce", act, grad, n, d, 1, B * (n - 1), gc_blocks((long)B * (n - 1), GC_MAX_BLOCKS), cam, minmax, workspace, stream);
}

extern "C" long nv_gradcam_per_volume_workspace_bytes(int B, int n) {
  if (B <= 0 || n <= 1) return -1;
  return gc_ticket_bytes(B) + 8L * B * gc_blocks(n - 1, GCV_MAX_BLOCKS);
}

extern "C" int nv_gradcam_reduce_per_volume(const void* act, const float* grad, int B, int n, int d, float* cam, float* minmax, void* workspace,
                                            long ws_bytes, void* stream) {
  NV_CHECK_ARG(act && grad && cam && workspace && B > 0 && B <= 65535 && n > 1 && d > 0 && (d % 8) == 0,
               "nv_gradcam_reduce_per_volume: bad arguments (d %% 8 == 0, n > 1, B <= 65535)");
  NV_CHECK_ARG(nv_aligned16(act) && nv_aligned16(grad) && nv_aligned16(workspace), "nv_gradcam_reduce_per_volume: 16-byte alignment");
  NV_CHECK_ARG(ws_bytes >= nv_gradcam_per_volume_workspace_bytes(B, n), "nv_gradcam_reduce_per_volume: workspace too small");
  return nv_attr_gradcam_launch("nv_gradcam_reduce_per_volume", act, grad, n, d, B, n - 1, gc_blocks(n - 1, GCV_MAX_BLOCKS), cam, minmax, workspace, stream);
}

extern "C" long nv_token_map_to_volume_workspace_bytes(int B, const int* grid3) {
  if (B <= 0 || !grid3 || grid3[0] <= 0 || grid3[1] <= 0 || grid3[2] <= 0) return -1;
  const long N = (long)grid3[0] * grid3[1] * grid3[2];
  return (2 * (long)B * N + B) * 4;
}

extern "C" int nv_token_map_to_volume(const float* maps, int B, const int* grid3, const int* out3, int normalize, double keep_percent, float* out,
                                      void* workspace, long ws_bytes, void* stream) {
  NV_CHECK_ARG(maps && grid3 && out3 && out && workspace && B > 0 && B <= 65535, "nv_token_map_to_volume: bad arguments (null pointer, or B outside [1, 65535])");
  const int G0 = grid3[0], G1 = grid3[1], G2 = grid3[2], S0 = out3[0], S1 = out3[1], S2 = out3[2];
  NV_CHECK_ARG(G0 > 0 && G1 > 0 && G2 > 0 && S0 > 0 && S1 > 0 && S2 > 0, "nv_token_map_to_volume: grid and output extents must be positive");
  const long N = (long)G0 * G1 * G2;
  NV_CHECK_ARG(N <= TM_MAX_CELLS, "nv_token_map_to_volume: grid %d x %d x %d has %ld cells, the kernel takes at most %d (16^3)", G0, G1, G2, N, TM_MAX_CELLS);
  NV_CHECK_ARG(keep_percent >= 0.0 && keep_percent <= 100.0, "nv_token_map_to_volume: keep_percent %g outside [0, 100]", keep_percent);
  const long lds = ((long)G1 * G2 + 2L * S1 + 2L * S2) * 4;
  NV_CHECK_ARG(lds <= 65536 && (long)S1 * S2 < (1L << 31),
               "nv_token_map_to_volume: output extents %d x %d x %d beyond the kernel's tables (G1 G2 + 2 S1 + 2 S2 <= 16384)", S0, S1, S2);
  NV_CHECK_ARG(nv_aligned16(out) && nv_aligned16(workspace) && nv_aligned(maps, 4), "nv_token_map_to_volume: out / workspace 16-byte aligned");
  NV_CHECK_ARG(ws_bytes >= nv_token_map_to_volume_workspace_bytes(B, grid3), "nv_token_map_to_volume: workspace too small");
  float* norm = (float*)workspace;
  float* sparse = norm + (long)B * N;
  float* cuts = sparse + (long)B * N;
  const int rc = nv_attr_threshold_launch("nv_token_map_to_volume (threshold)", maps, B, (int)N, normalize, keep_percent, norm, sparse, cuts, stream);
  if (rc != NV_OK) return rc;
  return nv_attr_upsample_launch("nv_token_map_to_volume (upsample)", sparse, B, grid3, out3, out, stream);
}

// ---- what series_attr.hip reuses (attr_common.h)
int nv_attr_gc_blocks(long rows, int groups) { return gc_blocks(rows, groups == 1 ? GC_MAX_BLOCKS : GCV_MAX_BLOCKS); }
long nv_attr_gc_workspace_bytes(int groups, int blocks) { return gc_ticket_bytes(groups) + 8L * groups * blocks; }

int nv_attr_threshold_launch(const char* name, const float* maps, int V, int N, int normalize, double keep_percent, float* norm, float* sparse, float* cuts,
                             void* stream) {
  hipLaunchKernelGGL(token_map_threshold_kernel, dim3(V), dim3(TM_THREADS), 0, (hipStream_t)stream, maps, N, normalize ? 1 : 0, quantile_pos(keep_percent, N),
                     norm, sparse, cuts);
  NV_CHECK_LAUNCH(name);
  return NV_OK;
}

int nv_attr_upsample_launch(const char* name, const float* sparse, int V, const int* grid3, const int* out3, float* out, void* stream) {
  const int G0 = grid3[0], G1 = grid3[1], G2 = grid3[2], S0 = out3[0], S1 = out3[1], S2 = out3[2];
  const long lds = ((long)G1 * G2 + 2L * S1 + 2L * S2) * 4;
  hipLaunchKernelGGL(upsample_trilinear_kernel, dim3(S0, V), dim3(UP_THREADS), (size_t)lds, (hipStream_t)stream, sparse, G0, G1, G2, S0, S1, S2,
                     (float)G0 / (float)S0, (float)G1 / (float)S1, (float)G2 / (float)S2, out);
  NV_CHECK_LAUNCH(name);
  return NV_OK;
}
