// Host-side checks of the classification-metric entry points (neurovit_amd/csrc/cls_metrics.hip) under the host sanitizers: argument
// refusals and the sizing helpers.  Every call carries bad arguments (or is host-only), so nothing is launched and no GPU is needed.
// Built by `make -C neurovit_amd/csrc cls-metrics-host-check` with -Xarch_host -fsanitize=address,undefined; run by
// tests/test_cls_metrics_cpu.py.
#define HOST_CHECK_NAME "cls_metrics_host_check"
#include "host_check.h"

int main() {
  alignas(16) double d[64] = {0};
  char* odd = reinterpret_cast<char*>(d) + 4;      // 4-byte but not 8-byte aligned
  // sizing
  EXPECT(nv_cls_metrics_state_doubles(2, 15) == NV_CLS_STATE_HEAD + 4 + 45);
  EXPECT(nv_cls_metrics_state_doubles(64, 64) == NV_CLS_STATE_HEAD + 4096 + 192);
  EXPECT(nv_cls_metrics_state_doubles(1, 15) == 0 && nv_cls_metrics_state_doubles(65, 15) == 0 && nv_cls_metrics_state_doubles(3, 0) == 0 && nv_cls_metrics_state_doubles(3, 65) == 0);
  EXPECT(nv_cls_metrics_table_floats(3) == NV_CLS_SCALARS + 15 + 9 && nv_cls_metrics_table_floats(1) == 0 && nv_cls_metrics_table_floats(65) == 0);
  EXPECT(nv_cls_auc_splits(8680, 2, 1) == 1 && nv_cls_auc_splits(1, 2, 0) == 1 && nv_cls_auc_splits(1, 2, 7) == 1);
  EXPECT(nv_cls_auc_splits(8680, 2, 0) == 17 && nv_cls_auc_splits(78820, 5, 0) == 4 && nv_cls_auc_splits(1000, 3, 3) == 2);      // (no empty split: 4 tiles in 3 -> 2 x 2)
  EXPECT(nv_cls_auc_splits(0, 2, 0) == 0 && nv_cls_auc_splits(NV_CLS_AUC_MAX_N + 1, 2, 0) == 0 && nv_cls_auc_splits(10, 1, 0) == 0 && nv_cls_auc_splits(10, 65, 0) == 0);
  EXPECT(nv_cls_auc_splits(10, 2, -1) == 0 && nv_cls_auc_splits(10, 2, NV_CLS_AUC_MAX_SPLITS + 1) == 0);
  EXPECT(nv_cls_auc_workspace_bytes(1000, 3, 1) == 1L * 4 * 3 * 2 * 8 && nv_cls_auc_workspace_bytes(1000, 3, 0) == 4L * 4 * 3 * 2 * 8);
  EXPECT(nv_cls_auc_workspace_bytes(NV_CLS_AUC_MAX_N, 64, 256) == 256L * (NV_CLS_AUC_MAX_N / 256) * 64 * 2 * 8);      // 64-bit arithmetic
  EXPECT(nv_cls_auc_workspace_bytes(0, 3, 1) == 0 && nv_cls_auc_workspace_bytes(10, 3, 300) == 0);
  // nv_cls_metrics_update: null pointers, B, C, bins, kind, lds, the state's alignment, the bank pairing and its window
  EXPECT(nv_cls_metrics_update(nullptr, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, nullptr, 4, 3, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, nullptr, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 0, 3, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 1, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 80, idx, 4, 65, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 0, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 65, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, 2, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 2, idx, 4, 3, 15, NV_CLS_LOGITS, d, nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, reinterpret_cast<double*>(odd), nullptr, 0, nullptr, 0, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, f, 4, nullptr, 0, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, nullptr, 4, idx, 0, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, f, 2, idx, 0, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, f, 4, idx, 5, 8, nullptr) == NV_ERR_ARG);      // row0 + B past the capacity
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, f, 4, idx, -1, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_update(f, 4, idx, 4, 3, 15, NV_CLS_LOGITS, d, f, 4, idx, 0x7fffffffffffffffL, 8, nullptr) == NV_ERR_ARG);      // no overflow in row0 + B
  EXPECT(strlen(nv_last_error()) > 0);
  // nv_cls_auc
  EXPECT(nv_cls_auc(nullptr, 4, idx, 8, 3, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, 1, d, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 0, 3, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, NV_CLS_AUC_MAX_N + 1, 3, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 1, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 80, idx, 8, 65, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 2, idx, 8, 3, 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, -1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, NV_CLS_AUC_MAX_SPLITS + 1, d, d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, 1, d, d, 47, nullptr) == NV_ERR_ARG);      // a workspace that is too small (48 bytes needed)
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, 1, reinterpret_cast<double*>(odd), d, 1024, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_auc(f, 4, idx, 8, 3, 1, d, odd, 1024, nullptr) == NV_ERR_ARG);
  // nv_segment_labels
  EXPECT(nv_segment_labels(nullptr, 4, idx, idx, 2, idx, idx, nullptr) == NV_ERR_ARG);
  EXPECT(nv_segment_labels(idx, 4, idx, idx, 2, idx, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_segment_labels(idx, 0, idx, idx, 2, idx, idx, nullptr) == NV_ERR_ARG);
  EXPECT(nv_segment_labels(idx, 4, idx, idx, 0, idx, idx, nullptr) == NV_ERR_ARG);
  // nv_cls_metrics_finish
  EXPECT(nv_cls_metrics_finish(nullptr, 3, 15, nullptr, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_finish(d, 3, 15, nullptr, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_finish(d, 1, 15, nullptr, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_finish(d, 3, 0, nullptr, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_finish(d, 3, 15, reinterpret_cast<double*>(odd), f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_cls_metrics_finish(reinterpret_cast<double*>(odd), 3, 15, nullptr, f, nullptr) == NV_ERR_ARG);
  return host_check_result();
}
