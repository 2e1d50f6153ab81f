// Host-side checks of the frozen-feature entry points (neurovit_amd/csrc/features.hip) under the host sanitizers: argument refusals,
// workspace sizing and the CSR validation.  Every call carries bad arguments (or is host-only), so nothing is launched and no GPU is needed.
// Built by `make -C neurovit_amd/csrc host-check` with -Xarch_host -fsanitize=address,undefined; run by tests/test_knn_cpu.py.
#include <vector>

#define HOST_CHECK_NAME "knn_host_check"
#include "host_check.h"

int main() {
  // nv_knn_topk: k, multiples of 4, alignment, group pairing, splits, workspace
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 8, 0, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 8, NV_KNN_MAX_K + 1, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 6, 2, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f + 1, 8, 4, f, 8, 4, 8, 2, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 4, 4, f, 8, 4, 8, 2, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 8, 2, idx, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 8, 2, nullptr, nullptr, 65, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 4, 8, 2, nullptr, nullptr, -1, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 200, 8, 2, nullptr, nullptr, 2, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 4, f, 8, 200, 8, 2, nullptr, nullptr, 2, idx, f, f, 8, nullptr) == NV_ERR_ARG);      // a workspace that is too small
  EXPECT(nv_knn_topk(nullptr, 8, 4, f, 8, 4, 8, 2, nullptr, nullptr, 0, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_topk(f, 8, 1 << 30, f, 8, 4, 8, 128, nullptr, nullptr, 1, idx, f, nullptr, 0, nullptr) == NV_ERR_ARG);      // Nq * k past 2^31
  EXPECT(strlen(nv_last_error()) > 0);
  // sizing
  EXPECT(nv_knn_topk_workspace_bytes(130, 1000, 20, 1) == 0);
  EXPECT(nv_knn_topk_workspace_bytes(130, 1000, 20, 3) == 3L * 130 * 20 * 8);
  EXPECT(nv_knn_topk_workspace_bytes(1 << 24, 1000, 128, 64) == 64L * (1 << 24) * 128 * 8);      // 64-bit arithmetic
  EXPECT(nv_knn_topk_workspace_bytes(130, 1000, 0, 3) == 0 && nv_knn_topk_workspace_bytes(130, 1000, 20, 65) == 0);
  EXPECT(nv_knn_topk_splits(8680, 78820, 0) == 8 && nv_knn_topk_splits(1, 3, 0) == 1 && nv_knn_topk_splits(1, 3, 7) == 7);
  EXPECT(nv_knn_topk_splits(0, 3, 0) == 0 && nv_knn_topk_splits(3, 0, 0) == 0 && nv_knn_topk_splits(3, 3, -1) == 0);
  EXPECT(nv_knn_topk_splits(2000000000, 2000000000, 0) == 1);
  // nv_pool_features
  EXPECT(nv_pool_features(f, 16, 8, 1, 1, 8, NV_POOL_PATCH_MEAN, 0, f, 8, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(f, 16, 8, 1, 2, 8, 3, 0, f, 8, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(f, 16, 4, 1, 2, 8, NV_POOL_CLS, 0, f, 8, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(f, 16, 8, 1, 2, 8, NV_POOL_CLS, 0, f, 4, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(f, 16, 8, 1, 2, 8, NV_POOL_CLS, 0, f, 8, -1, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(f, 16, 8, 1, 2, 1 << 20, NV_POOL_CLS, 0, f, 1 << 20, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_pool_features(nullptr, 16, 8, 1, 2, 8, NV_POOL_CLS, 0, f, 8, 0, nullptr) == NV_ERR_ARG);
  // nv_knn_vote
  EXPECT(nv_knn_vote(idx, f, 4, 8, 9, NV_KNN_UNIFORM, 0.07f, 8, idx, 3, f, idx, nullptr, 0, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 129, 8, NV_KNN_UNIFORM, 0.07f, 8, idx, 3, f, idx, nullptr, 0, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, 2, 0.07f, 8, idx, 3, f, idx, nullptr, 0, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, NV_KNN_SOFTMAX, 0.f, 8, idx, 3, f, idx, nullptr, 0, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, NV_KNN_UNIFORM, 0.07f, 8, idx, 3, f, idx, f, 2, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, NV_KNN_UNIFORM, 0.07f, 8, nullptr, 3, f, idx, nullptr, 2, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, NV_KNN_UNIFORM, 0.07f, 8, idx, 0, f, idx, nullptr, 0, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_knn_vote(idx, f, 4, 8, 8, NV_KNN_UNIFORM, 0.07f, 8, nullptr, 0, nullptr, nullptr, f, 2, nullptr, nullptr) == NV_ERR_ARG);
  // the CSR: exactly-sized heap arrays, so a read past either end is caught
  {
    std::vector<int> order = {3, 0, 2, 1}, offsets = {0, 1, 1, 4};
    EXPECT(nv_segment_csr_check(order.data(), offsets.data(), 4, 3) == NV_OK);
    std::vector<int> dec = {0, 3, 2, 4};
    EXPECT(nv_segment_csr_check(order.data(), dec.data(), 4, 3) == NV_ERR_ARG);
    std::vector<int> from1 = {1, 2, 3, 4};
    EXPECT(nv_segment_csr_check(order.data(), from1.data(), 4, 3) == NV_ERR_ARG);
    std::vector<int> past = {0, 1, 2, 5};
    EXPECT(nv_segment_csr_check(order.data(), past.data(), 4, 3) == NV_ERR_ARG);
    std::vector<int> neg = {-1, 1, 2, 4};
    EXPECT(nv_segment_csr_check(order.data(), neg.data(), 4, 3) == NV_ERR_ARG);
    std::vector<int> bad_order = {3, 0, 4, 1};
    EXPECT(nv_segment_csr_check(bad_order.data(), offsets.data(), 4, 3) == NV_ERR_ARG);
    std::vector<int> partial = {0, 1, 1, 2}, short_order = {3, 0};      // offsets may stop short of N: only order[0 .. offsets[G]) is read
    EXPECT(nv_segment_csr_check(short_order.data(), partial.data(), 4, 3) == NV_OK);
    EXPECT(nv_segment_csr_check(nullptr, offsets.data(), 4, 3) == NV_ERR_ARG);
    EXPECT(nv_segment_csr_check(order.data(), offsets.data(), 4, 0) == NV_ERR_ARG);
  }
  EXPECT(nv_segment_mean(f, 4, 4, 8, idx, idx, 2, f, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_segment_mean(f, 8, 4, 8, idx, idx, 70000, f, 8, nullptr) == NV_ERR_ARG);
  EXPECT(nv_segment_mean(f, 8, 4, 8, nullptr, idx, 2, f, 8, nullptr) == NV_ERR_ARG);
  return host_check_result();
}
