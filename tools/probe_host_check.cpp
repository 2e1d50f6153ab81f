// Host-side checks of the linear-probe entry points (neurovit_amd/csrc/probe.hip) under the host sanitizers: argument refusals and workspace
// sizing.  Every call carries bad arguments (or is host-only), so nothing is launched and no GPU is needed.
// Built by `make -C neurovit_amd/csrc probe-host-check` with -Xarch_host -fsanitize=address,undefined; run by tests/test_probe_cpu.py.
#define HOST_CHECK_NAME "probe_host_check"
#include "host_check.h"

static nv_probe_heads heads(int H, int C) {
  nv_probe_heads h;
  memset(&h, 0, sizeof h);
  h.struct_size = (int)sizeof h;
  h.H = H;
  h.C = C;
  return h;
}

int main() {
  alignas(16) double dbl[64] = {0};
  int lab[64] = {0};
  alignas(16) char ws[1 << 16];
  const long big = sizeof ws;
  // sizing: nchunks * (M d floats + 2 * 32 doubles); 64-bit arithmetic; 0 for what nv_probe_grad refuses
  EXPECT(nv_probe_grad_workspace_bytes(517, 72, 15) == 3L * (15 * 72 * 4 + 512));
  EXPECT(nv_probe_grad_workspace_bytes(256, 4, 1) == 1L * (16 + 512) && nv_probe_grad_workspace_bytes(257, 4, 1) == 2L * (16 + 512));
  EXPECT(nv_probe_grad_workspace_bytes(2000000000, 1024, 32) == 7812500L * (32L * 1024 * 4 + 512));
  EXPECT(nv_probe_grad_workspace_bytes(0, 72, 15) == 0 && nv_probe_grad_workspace_bytes(517, 70, 15) == 0 && nv_probe_grad_workspace_bytes(517, 1028, 15) == 0);
  EXPECT(nv_probe_grad_workspace_bytes(517, 72, 33) == 0 && nv_probe_grad_workspace_bytes(517, 72, 0) == 0 && nv_probe_grad_workspace_bytes(517, 0, 4) == 0);
  EXPECT(nv_probe_stats_workspace_bytes(517, 72) == (2L * 3 * 72 + 2 * 72 + 3) * 8 && nv_probe_stats_workspace_bytes(517, 0) == 3 * 8);
  EXPECT(nv_probe_stats_workspace_bytes(0, 72) == 0 && nv_probe_stats_workspace_bytes(517, -1) == 0);
  // nv_probe_grad: the heads, M, d, ld, alignment, task and NULL combinations, the workspace
  nv_probe_heads ok = heads(2, 3), wide = heads(3, 11), none = heads(0, 3), wrong = heads(2, 3), neg = heads(2, 3);
  wrong.struct_size = 8;
  neg.l2[1] = -1.f;
#define GRAD(X, ldx, N, d, mean, rstd, W, b, hd, task, labels, cw, targets, tm, ts, denom, dW, db, loss, mb, wsp, wsb) \
  nv_probe_grad(X, ldx, N, d, mean, rstd, W, b, hd, task, labels, cw, targets, tm, ts, denom, dW, db, loss, mb, wsp, wsb, nullptr)
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, nullptr, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &wrong, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &wide, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);      // M = 33
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &none, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &neg, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 6, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);        // d % 4
  EXPECT(GRAD(f, 1028, 4, 1028, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);  // d > 1024
  EXPECT(GRAD(f, 8, 4, 0, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 4, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);        // ldx < d
  EXPECT(GRAD(f, 10, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);       // ldx % 4
  EXPECT(GRAD(f + 1, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);    // alignment
  EXPECT(GRAD(f, 8, 4, 8, f, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);              // mean without rstd
  EXPECT(GRAD(f, 8, 0, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(nullptr, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, nullptr, f, f, f, 0, ws, big) == NV_ERR_ARG);    // no denominators
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, nullptr, 0, ws, big) == NV_ERR_ARG);
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 2, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);        // task
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, nullptr, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);    // no labels
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, f, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);              // labels and targets
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, f, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);              // target_mean in classification
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 1, nullptr, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);    // no targets
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 1, nullptr, f, f, nullptr, nullptr, dbl, f, f, f, 0, ws, big) == NV_ERR_ARG);                // class_weight in regression
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, -1, ws, big) == NV_ERR_ARG);       // max_blocks
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, nullptr, 0) == NV_ERR_ARG);     // no workspace
  EXPECT(GRAD(f, 8, 4, 8, nullptr, nullptr, f, f, &ok, 0, lab, nullptr, nullptr, nullptr, nullptr, dbl, f, f, f, 0, ws, 8) == NV_ERR_ARG);          // too small
  EXPECT(strlen(nv_last_error()) > 0);
  // nv_probe_step
  EXPECT(nv_probe_step(f, f, f, f, f, f, f, f, 8, nullptr, 0.9f, 0.999f, 0.1f, 0.001f, 0.03f, 1e-8f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_step(f, f, f, f, f, f, f, f, 8, &wrong, 0.9f, 0.999f, 0.1f, 0.001f, 0.03f, 1e-8f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_step(f, f, f, f, f, nullptr, f, f, 8, &ok, 0.9f, 0.999f, 0.1f, 0.001f, 0.03f, 1e-8f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_step(f, f, f, f, f, f, f, f, 0, &ok, 0.9f, 0.999f, 0.1f, 0.001f, 0.03f, 1e-8f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_step(f, f, f, f, f, f, f, f, 8, &ok, 1.0f, 0.999f, 0.1f, 0.001f, 0.03f, 1e-8f, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_step(f, f, f, f, f, f, f, f, 8, &ok, 0.9f, 0.999f, 0.1f, 0.001f, 0.f, 1e-8f, nullptr) == NV_ERR_ARG);
  // nv_probe_predict
  EXPECT(nv_probe_predict(f, 8, 4, 8, nullptr, nullptr, f, f, 3, 11, f, 33, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_predict(f, 8, 4, 8, nullptr, nullptr, f, f, 2, 3, f, 4, nullptr, 0, nullptr) == NV_ERR_ARG);           // ldl < M
  EXPECT(nv_probe_predict(f, 8, 4, 8, nullptr, nullptr, f, f, 2, 3, f, 6, f, 4, nullptr) == NV_ERR_ARG);                 // ldp < M
  EXPECT(nv_probe_predict(f, 8, 4, 6, nullptr, nullptr, f, f, 2, 3, f, 6, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_predict(f, 8, 4, 8, nullptr, f, f, f, 2, 3, f, 6, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_predict(f, 8, 4, 8, nullptr, nullptr, f, f, 2, 3, nullptr, 6, nullptr, 0, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_predict(f, 8, 0, 8, nullptr, nullptr, f, f, 2, 3, f, 6, nullptr, 0, nullptr) == NV_ERR_ARG);
  // nv_probe_stats
  EXPECT(nv_probe_stats(nullptr, 0, 4, 0, 0, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);   // nothing asked
  EXPECT(nv_probe_stats(f, 8, 4, 0, 0, 0.f, f, f, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);                   // X with d = 0
  EXPECT(nv_probe_stats(f, 4, 4, 8, 0, 0.f, f, f, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);                   // ldx < d
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);       // no output
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, -1.f, f, f, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, 0.f, f, f, nullptr, nullptr, lab, 2, nullptr, nullptr, ws, big, nullptr) == NV_ERR_ARG);                       // labels without denom
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, 0.f, f, f, nullptr, nullptr, nullptr, 2, f, nullptr, ws, big, nullptr) == NV_ERR_ARG);                         // class_weight without labels
  EXPECT(nv_probe_stats(nullptr, 0, 4, 0, 0, 0.f, nullptr, nullptr, nullptr, nullptr, lab, 0, nullptr, dbl, ws, big, nullptr) == NV_ERR_ARG);         // C = 0
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, 0.f, f, f, nullptr, nullptr, nullptr, 0, nullptr, nullptr, ws, 8, nullptr) == NV_ERR_ARG);                     // workspace too small
  EXPECT(nv_probe_stats(f, 8, 4, 8, 0, 0.f, f, f, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) == NV_ERR_ARG);
  return host_check_result();
}
