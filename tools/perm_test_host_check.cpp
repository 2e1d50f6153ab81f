// Host-side checks of the permutation-test entry points (neurovit_amd/csrc/perm_test.hip) under the host sanitizers: argument refusals and
// the sizing helpers.  Every call carries bad arguments (or is host-only), so nothing is launched and no GPU is needed.
// Built by `make -C neurovit_amd/csrc perm-test-host-check` with -Xarch_host -fsanitize=address,undefined; run by
// tests/test_perm_test_cpu.py.
#define HOST_CHECK_NAME "perm_test_host_check"
#include "host_check.h"

int main() {
  alignas(16) float ws[64] = {0};
  unsigned char mask[64] = {0};
  const double alphas[2] = {0.05, 0.01}, bad_alpha[1] = {1.0}, zero_alpha[1] = {0.0};
  float* odd = f + 1;      // 4-byte but not 16-byte aligned
  const int ONE = NV_PERM_ONE_SAMPLE, TWO = NV_PERM_TWO_SAMPLE;
  // sizing: splits never exceed the row tiles, no split is empty, the automatic choice aims at 1024 workgroups
  EXPECT(nv_perm_splits(10000, 1000, 0) == 53 && nv_perm_splits(10000, 729000, 0) == 1 && nv_perm_splits(32, 130, 0) == 1 && nv_perm_splits(512, 130, 3) == 3);
  EXPECT(nv_perm_splits(100, 40, 3) == 2 && nv_perm_splits(1, 1, 0) == 1 && nv_perm_splits(1 << 20, 512, 256) == 256);
  EXPECT(nv_perm_splits(0, 10, 0) == 0 && nv_perm_splits(NV_PERM_MAX_R + 1, 10, 0) == 0 && nv_perm_splits(10, 0, 0) == 0 && nv_perm_splits(10, 10, -1) == 0 &&
         nv_perm_splits(10, 10, NV_PERM_MAX_SPLITS + 1) == 0);
  EXPECT(nv_perm_workspace_bytes(32, 130, 1) == 4L * (4 + 132 + 132 + 32 * 3));
  EXPECT(nv_perm_workspace_bytes(512, 130, 3) == 4L * (4 + 132 + 392 + 512 * 3));
  EXPECT(nv_perm_workspace_bytes(1 << 20, 729000, 1) == 4L * (2848 + 729000 + 729000 + (1L << 20) * 11391));      // 64-bit arithmetic
  EXPECT(nv_perm_workspace_bytes(0, 130, 1) == 0 && nv_perm_workspace_bytes(32, 130, 300) == 0);
  EXPECT(nv_perm_rank(0.05, 100) == 95 && nv_perm_rank(0.01, 100) == 99 && nv_perm_rank(0.05, 32) == 31 && nv_perm_rank(0.01, 32) == 32 && nv_perm_rank(0.05, 10000) == 9500);
  EXPECT(nv_perm_rank(0.0, 100) == 0 && nv_perm_rank(1.0, 100) == 0 && nv_perm_rank(0.5, 0) == 0);
  // nv_perm_design: kind, N, the groups, R, exact enumeration, M
  EXPECT(nv_perm_design(2, 8, 0, nullptr, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 1, 0, nullptr, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, NV_PERM_MAX_N + 1, 0, nullptr, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 8, 0, nullptr, 0, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 8, 0, nullptr, NV_PERM_MAX_R + 1, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 8, 0, nullptr, 16, 0, 1, nullptr, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 8, 0, nullptr, 16, 0, 1, odd, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(ONE, 21, 0, nullptr, 1 << 20, 1, 1, f, nullptr) == NV_ERR_ARG);      // 2^21 rows
  EXPECT(nv_perm_design(ONE, 5, 0, nullptr, 31, 1, 1, f, nullptr) == NV_ERR_ARG);            // exact needs R = 2^N
  EXPECT(nv_perm_design(TWO, 7, 3, idx, 128, 1, 1, f, nullptr) == NV_ERR_ARG);               // no exact two-sample enumeration
  EXPECT(nv_perm_design(TWO, 2, 1, idx, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(TWO, 7, 0, idx, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(TWO, 7, 7, idx, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_design(TWO, 7, 3, nullptr, 16, 0, 1, f, nullptr) == NV_ERR_ARG);
  EXPECT(strlen(nv_last_error()) > 0);
  // nv_perm_stats
  EXPECT(nv_perm_stats(nullptr, 8, 5, 8, ONE, 0, nullptr, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_stats(f, 8, 5, 8, ONE, 0, nullptr, mask, f, f, f, nullptr, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_stats(f, 8, 5, 8, ONE, 0, nullptr, mask, f, f, f, idx, nullptr, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_stats(f, 8, 1, 8, ONE, 0, nullptr, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_stats(f, 8, 5, 0, ONE, 0, nullptr, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_stats(f, 7, 5, 8, ONE, 0, nullptr, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);      // ldx < V
  EXPECT(nv_perm_stats(f, 8, 5, 8, TWO, 2, nullptr, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);      // two samples without labels
  EXPECT(nv_perm_stats(f, 8, 5, 8, TWO, 5, idx, mask, f, f, f, idx, ws, 256, nullptr) == NV_ERR_ARG);          // an empty group
  EXPECT(nv_perm_stats(f, 8, 5, 8, ONE, 0, nullptr, mask, f, f, f, idx, ws, 3, nullptr) == NV_ERR_ARG);        // a workspace that is too small
  EXPECT(nv_perm_stats(f, 8, 5, 8, ONE, 0, nullptr, mask, f, f, f, idx, odd, 256, nullptr) == NV_ERR_ARG);
  // nv_perm_maxstat
  EXPECT(nv_perm_maxstat(nullptr, 8, 5, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, nullptr, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 1, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, NV_PERM_MAX_N + 1, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 0, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, NV_PERM_MAX_R + 1, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 7, 5, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 32, f, f, 3, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 32, f, f, NV_PERM_TAIL_LESS, -1, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 32, f, f, NV_PERM_TAIL_LESS, NV_PERM_MAX_SPLITS + 1, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, odd, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_maxstat(f, 8, 5, 8, f, 32, f, f, NV_PERM_TAIL_TWO, 0, ws, nv_perm_workspace_bytes(32, 8, 0) - 1, nullptr) == NV_ERR_ARG);
  // nv_perm_finish
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, nullptr, alphas, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, f, nullptr, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(3, 5, 32, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(TWO, 2, 32, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 0, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 0, 0, f, alphas, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, alphas, NV_PERM_MAX_ALPHAS + 1, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, nullptr, 2, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, nullptr, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, bad_alpha, 1, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, zero_alpha, 1, f, f, idx, idx, f, f, f, ws, 256, nullptr) == NV_ERR_ARG);
  EXPECT(nv_perm_finish(ONE, 5, 32, 8, 0, f, alphas, 2, f, f, idx, idx, f, f, f, ws, nv_perm_workspace_bytes(32, 8, 0) - 1, nullptr) == NV_ERR_ARG);
  return host_check_result();
}
