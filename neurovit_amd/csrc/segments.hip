// Segments of rows (the volumes of a subject) as a CSR table: its host-side validation (nv_segment_csr_check), per-segment means
// (nv_segment_mean) and per-segment labels (nv_segment_labels).  The definitions are in the header.  Nothing here reads back, nothing uses
// atomics; every sum has one fixed order, so the bits reproduce from run to run.
#include "eval_common.h"

namespace {

__global__ __launch_bounds__(256) void segment_mean_kernel(const float* __restrict__ src, long lds, int N, int w, const int* __restrict__ order,
                                                           const int* __restrict__ offsets, float* __restrict__ out, long ldo) {
  const int gseg = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= w) return;
  double s = 0.0;
  int cnt = 0;
  segment_rows(order, offsets, gseg, N, [&](int r) {
    s += (double)src[(long)r * lds + c];
    ++cnt;
  });
  out[(long)gseg * ldo + c] = cnt > 0 ? (float)(s / (double)cnt) : 0.f;
}

__global__ __launch_bounds__(256) void segment_labels_kernel(const int* __restrict__ labels, int N, const int* __restrict__ order, const int* __restrict__ offsets,
                                                             int G, int* __restrict__ out, int* __restrict__ mixed) {
  __shared__ int red[1][4];
  int cnt = 0;
  for (int g = threadIdx.x; g < G; g += 256) {
    int first = -1, differ = 0;
    bool have = false;
    segment_rows(order, offsets, g, N, [&](int r) {
      const int l = labels[r];
      if (!have) { first = l; have = true; }
      else if (l >= 0 && l != first) differ = 1;
    });
    out[g] = have ? first : -1;
    cnt += differ;
  }
  cnt = block_sum4(cnt, red);
  if (threadIdx.x == 0) mixed[0] = cnt;
}

}  // namespace

extern "C" int nv_segment_csr_check(const int* order, const int* offsets, int N, int G) {
  NV_CHECK_ARG(order && offsets && N > 0 && G > 0, "nv_segment_csr_check: null pointer or bad shape N=%d G=%d", N, G);
  NV_CHECK_ARG(offsets[0] == 0 && offsets[G] <= N, "nv_segment_csr_check: offsets must run from 0 to at most N=%d, got %d .. %d", N, offsets[0], offsets[G]);
  for (int gseg = 0; gseg < G; ++gseg)
    NV_CHECK_ARG(offsets[gseg] <= offsets[gseg + 1], "nv_segment_csr_check: offsets decrease at segment %d (%d > %d)", gseg, offsets[gseg], offsets[gseg + 1]);
  for (int p = 0; p < offsets[G]; ++p) NV_CHECK_ARG(order[p] >= 0 && order[p] < N, "nv_segment_csr_check: order[%d] = %d outside [0, %d)", p, order[p], N);
  return NV_OK;
}

extern "C" int nv_segment_mean(const float* src, long lds, int N, int w, const int* order, const int* offsets, int G, float* out, long ldo, void* stream) {
  NV_CHECK_ARG(src && order && offsets && out && N > 0 && w > 0 && G > 0, "nv_segment_mean: null pointer or bad shape N=%d w=%d G=%d", N, w, G);
  NV_CHECK_ARG(lds >= w && ldo >= w && G <= 65535, "nv_segment_mean: lds=%ld and ldo=%ld must cover w=%d; at most 65535 segments per call, got %d", lds, ldo, w, G);
  hipLaunchKernelGGL(segment_mean_kernel, dim3((w + 255) / 256, G), dim3(256), 0, (hipStream_t)stream, src, lds, N, w, order, offsets, out, ldo);
  NV_CHECK_LAUNCH("nv_segment_mean");
  return NV_OK;
}

extern "C" int nv_segment_labels(const int* labels, int N, const int* order, const int* offsets, int G, int* out, int* mixed, void* stream) {
  NV_CHECK_ARG(labels && order && offsets && out && mixed && N >= 1 && G >= 1, "nv_segment_labels: null pointer or bad shape N=%d G=%d", N, G);
  NV_CHECK_ARG(nv_aligned(labels, 4) && nv_aligned(order, 4) && nv_aligned(offsets, 4) && nv_aligned(out, 4) && nv_aligned(mixed, 4), "nv_segment_labels: every array 4-byte aligned");
  hipLaunchKernelGGL(segment_labels_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, labels, N, order, offsets, G, out, mixed);
  NV_CHECK_LAUNCH("nv_segment_labels");
  return NV_OK;
}
