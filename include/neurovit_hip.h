/* neurovit_hip.h - C ABI of libneurovit_hip.so: the MI355X (gfx950) hot path of NeuroViT.
 *
 * The reference (gillet-thomas/NeuroViT) has NO native/FFI interface: its seam is the Python
 * nn.Module contract.  This header is the C-ABI that sits beneath our drop-in
 * nn.Modules; every entry point names the reference code it replaces (paths relative to the
 * reference checkout).  The Python binding a maintainer adds is a ctypes.CDLL stub - see
 * INTEGRATION.md.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes, no torch types; `void*` buffers marked bf16 hold bfloat16;
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch owns all memory);
 *   - `stream` is a hipStream_t; nothing here allocates, frees or synchronises;
 *   - returns 0 on success, <0 on error (NV_ERR_*); nv_last_error() gives the message;
 *   - row-major, `ld*` = leading dimension in ELEMENTS;
 *   - arithmetic: bf16 MFMA operands, fp32 accumulate, fp32 residual stream / LayerNorm /
 *     softmax / optimizer state ("dtype": "bf16" in bench.py).
 */
#ifndef NEUROVIT_HIP_H
#define NEUROVIT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define NV_OK 0
#define NV_ERR_ARG (-1)
#define NV_ERR_HIP (-2)
#define NV_ERR_ARCH (-3)

/* ---- housekeeping ------------------------------------------------------------------------- */
int nv_version(void);
int nv_arch_ok(void);                 /* 1 iff the current HIP device is gfx950 */
const char* nv_last_error(void);

/* ---- 16-bit operand format (process-wide, like the nv_*_set_* tuning switches): what every `void*` buffer this header calls
 * "bf16" holds, and which MFMA instruction contracts it.  NV_OPERAND_BF16 (default; BASELINE.json's dtype) or NV_OPERAND_FP16 - the
 * reference's own training arithmetic (torch.autocast(float16) + GradScaler, src/Trainer.py:29,68,74-76): same MFMA rate, 11 instead
 * of 8 significand bits (logits within 1e-3 of the reference's fp32 CPU forward), 5 instead of 8 exponent bits (train with a loss
 * scale: nv_train_hparams.loss_scale).  The fp8 entry points require NV_OPERAND_BF16.  Set it before the calls of a model; buffers
 * written under one format must be read under the same one. */
#define NV_OPERAND_BF16 0
#define NV_OPERAND_FP16 1
int nv_set_operand_format(int fmt);
int nv_operand_format(void);

/* ---- optional per-launch hipEvent profiler (bench.py roofline leg).  kind: warp-specialised GEMM kernels 0 NT, 1 NN, 2 TN;
 * 3 attention fwd, 4 attention bwd; 5 fp8 GEMM; eight-wave 256 x 128 GEMM kernel 10 NT, 11 NN, 12 TN, 13 grouped TN; 256 x 256 kernel 20 NT,
 * 21 NN, 22 TN; fp32 path: 30 GEMM, 31 attention.  nv_prof_summary synchronises; call it outside timed regions. */
int nv_prof_enable(int on);
int nv_prof_summary(int kind, double* ms, double* work, long* count);
int nv_prof_summary_bytes(int kind, double* bytes);   /* algorithmic bytes (operands read once + outputs written once) of the same records */

/* ---- GEMM with fused epilogues (replaces every nn.Linear on the path: vit_3d.py:19,22,41,44,94)
 * layout 0 (NT): C[M,N] = A[M,K] . B[N,K]^T      forward  y = x W^T
 * layout 1 (NN): C[M,N] = A[M,K] . B[K,N]        dgrad    dx = dy W
 * layout 2 (TN): C[M,N] = A[K,M]^T . B[K,N]      wgrad    dW = dy^T x
 * epi 0 STORE_BF16, 1 STORE_F32 (+= if accumulate), 2 BIAS_F32, 3 BIAS_GELU (aux_out = pre-activation bf16,
 * C = exact-erf GELU bf16; vit_3d.py:19-20), 4 BIAS_RESID (C f32 = aux_in f32 + acc + bias; vit_3d.py:73-74),
 * 5 DGELU (C bf16 = acc * gelu'(aux_in bf16)), 6 DGELU_COLSUM (5, and aux_out f32 [ceil(M / tile rows), ld_aux_out] receives the
 * per-tile column sums of the stored values: the bias gradient of the Linear in front of the GELU without a second pass over C;
 * sum its rows with nv_reduce_multi; tile rows from nv_gemm_tile_rows).  A, B bf16.
 * Dropout (nn.Dropout of vit_3d.py:21,23,45; drop_p = 0 disables): applied by epilogue 3 to the GELU output, by 4 to
 * (acc + bias) before the residual add, by 5 to acc; element (m, n) is kept iff hash(drop_seed, m*N + n) >= p*2^32 and
 * scaled by 1/(1-p) - the same mask is recomputed wherever the backward pass needs it. */
/* epilogue 1 (fp32 store / accumulate): aux_out, when given, receives a bf16 copy of the stored values (ld_aux_out elements per row) */
int nv_gemm_bf16(int layout, int epi, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C,
                 long ldc, const float* bias, const void* aux_in, long ld_aux_in, void* aux_out, long ld_aux_out,
                 int accumulate, float alpha, unsigned long drop_seed, float drop_p, void* stream);

int nv_gemm_tile_rows(int layout, int M, int N, int K, long lda, long ldb);   /* 0: epilogue 6 not available for this shape */

/* ---- fp8 inference path (BASELINE.json configs[4]: ViT3D-large, "fp8 MFMA"): OCP e4m3 operands, fp32 accumulate on
 * v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales), dequantisation per output column in the epilogue.
 * nv_quant_rows_f8: out8[r, :] = sat(W[r, :] * sw[r]) with sw[r] = 448 / max|W[r, :]|; colscale[r] = 1 / (act_scale * sw[r]).
 * nv_ln_fwd_f8: LayerNorm(d) (vit_3d.py:18,37) -> sat(y * out_scale) as e4m3 (inference: no statistics saved).
 * nv_gemm_f8 (NT): C = epi((A8 . B8^T) * colscale[n]); epi 0 bf16 store, 1 f32 store, 4 f32 = aux_in + acc + bias,
 * 7 e4m3 = sat(gelu(acc + bias) * out_scale) (FC1 feeding FC2).  K % 128 == 0.
 * sat: finite values and infinities beyond +-448 become +-448 (0x7E / 0xFE); a NaN stays a NaN (0x7F / 0xFF) in every e4m3 writer. */
int nv_quant_rows_f8(const float* W, long ldw, int rows, int cols, void* out8, long ld8, float act_scale, float* colscale, void* stream);
int nv_ln_fwd_f8(const float* x, long ldx, int M, int d, const float* gamma, const float* beta, float eps, float out_scale, void* y8,
                 long ldy, void* stream);
int nv_gemm_f8(int epi, int M, int N, int K, const void* A8, long lda, const void* B8, long ldb, void* C, long ldc,
               const float* colscale, const float* bias, const void* aux_in, long ld_aux_in, float out_scale, void* stream);
/* Training forward on fp8 operands (BASELINE.json configs[4], "fwd / fwd+bwd"): the forward linears run on e4m3 operands, the backward
 * pass stays on bf16 operands and reads bf16 copies that the SAME forward kernels write.
 * nv_ln_fwd_f8_train: nv_ln_fwd_f8 + the bf16 output and the row statistics of nv_ln_fwd (bit for bit) in one pass over x.
 * nv_gemm_f8_gelu_train (FC1): h8 e4m3 = sat(gelu(u) * out_scale), h16 bf16 = gelu(u), u16 bf16 (optional) = u = acc * colscale + bias. */
int nv_ln_fwd_f8_train(const float* x, long ldx, int M, int d, const float* gamma, const float* beta, float eps, float out_scale, void* y8, long ldy8,
                       void* y16, long ldy16, float* mean, float* rstd, void* stream);
int nv_gemm_f8_gelu_train(int M, int N, int K, const void* A8, long lda, const void* B8, long ldb, const float* colscale, const float* bias,
                          float out_scale, void* h8, long ldh8, void* h16, long ldh16, void* u16, long ldu16, unsigned long drop_seed,
                          float drop_p, void* stream);      /* dropout (vit_3d.py:21) on gelu(u): h8 and h16 carry the same mask */
/* nv_gemm_f8 epilogue 4 with the nn.Dropout of vit_3d.py:23 on (acc * colscale + bias) before the residual add (mask of nv_gemm_bf16 epilogue 4) */
int nv_gemm_f8_resid_drop(int M, int N, int K, const void* A8, long lda, const void* B8, long ldb, void* C, long ldc, const float* colscale,
                          const float* bias, const void* aux_in, long ld_aux_in, unsigned long drop_seed, float drop_p, void* stream);

/* ---- fp32 inference path ("precise" mode).  The reference validates in fp32 without autocast (src/Trainer.py:101-118) and the logits
 * are to match its CPU forward to 1e-3; bf16 MFMA operands cannot (weights rounded to bf16 alone cost 1e-3 ... 6e-3), so these entry
 * points keep every operand fp32 and contract on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains, 1/16 of the bf16 MFMA rate).
 * nv_gemm_f32 (NT only: every nn.Linear forward, vit_3d.py:19,22,41,44,94): C[M,N] = epi(A[M,K] . B[N,K]^T), all fp32, B = the
 * [out, in] weight as the state_dict holds it.  epi 0 store, 2 + bias, 3 exact-erf GELU(+ bias), 4 resid + (+ bias).  N % 4 == 0.
 * Any K / lda / ldb (float4 operand loads when they are multiples of 4 and 16-byte aligned, scalar loads otherwise).
 * nv_attn_fwd_f32 (vit_3d.py:53-59): qkv f32 [B, n, 3*inner] -> out f32 [B, n, inner]; dim_head a multiple of 4 up to 128. */
int nv_gemm_f32(int epi, int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                const float* bias, const float* resid, long ldr, void* stream);
int nv_gemm_f32_set_tile(int wm, int wn);     /* tuning aid: wave tile (16 wm) x (16 wn), wm, wn in {2, 4}; (0, 0) = heuristic; (-1, 2 | 4 | 0): waves per workgroup of nv_attn_fwd_f32 */
int nv_attn_fwd_f32(const float* qkv, long ld_qkv, int B, int n, int heads, int dim_head, float scale, float* out, long ld_out,
                    void* stream);
int nv_ln_fwd_f32(const float* x, long ldx, int M, int d, const float* gamma, const float* beta, float eps, float* y, long ldy,
                  float* mean, float* rstd, void* stream);      /* as nv_ln_fwd with an fp32 output; mean / rstd may both be NULL */

/* Up to four independent problems of one layout / epilogue in ONE launch (provided for layout 2 / TN with epilogue 1: the
 * four weight-gradient GEMMs of a transformer layer, vit_3d.py:19,22,41,44 backward).  Same arithmetic per tile as
 * nv_gemm_bf16; the point is occupancy: 864 tiles together instead of 72-288 at a time. */
typedef struct nv_gemm_problem {
  int M, N, K;
  const void* A; long lda;     /* A[K, M] bf16 (layout 2) */
  const void* B; long ldb;     /* B[K, N] bf16 */
  void* C; long ldc;           /* C[M, N] f32 */
  int accumulate;              /* C += instead of C = */
  void* C16; long ldc16;       /* optional (NULL): bf16 mirror of the stored C (data-parallel gradient message) */
} nv_gemm_problem;
int nv_gemm_bf16_grouped(int layout, int epi, int count, const nv_gemm_problem* problems, void* stream);

/* ---- AdamW applied where the gradient is produced (Trainer.py:75 optimizer.step() folded into loss.backward() for the Linear
 * weights: torch's "optimizer in backward" pattern).  The five arenas share element offsets: element i of `grads` is the gradient of
 * params[i], whose optimizer state is adam_m[i] / adam_v[i] and whose bf16 shadow is params16[i].
 * nv_gemm_bf16_grouped_adamw: the TN problems of nv_gemm_bf16_grouped (every C inside `grads`, accumulate = 0, no C16) whose epilogue
 *   runs the update of nv_adamw_step on the tile it holds instead of storing it - the same arithmetic on the same fp32 gradient, so
 *   parameters, state and shadow come out bit-identical to nv_gemm_bf16_grouped + nv_adamw_step; the gradient itself is stored only
 *   when keep_grads = 1.  26 B/param of memory traffic instead of 34, and no second pass over these weights.
 *   The caller orders every reader of the weights' bf16 shadow (the data-gradient GEMMs of the same layer) BEFORE this launch.
 * nv_adamw_ranges: the plain update (nv_adamw_step arithmetic, fp32 gradients) over `count` element ranges (HOST arrays; begins and
 *   lens multiples of 4) in one launch - the rest of the arena (biases, LayerNorm, embeddings, head) behind a fused backward. */
typedef struct nv_adamw_arena {
  int struct_size;            /* sizeof(nv_adamw_arena) */
  int step;                   /* >= 1 */
  double lr, beta1, beta2, eps, weight_decay;
  float grad_scale;           /* the update reads grad * grad_scale */
  int keep_grads;             /* nv_gemm_bf16_grouped_adamw: 1 = also store the gradient to C */
  float* params; float* grads; float* adam_m; float* adam_v; void* params16;
} nv_adamw_arena;
int nv_gemm_bf16_grouped_adamw(int count, const nv_gemm_problem* problems, const nv_adamw_arena* opt, void* stream);
int nv_adamw_ranges(const nv_adamw_arena* opt, const long* begins, const long* lens, int count, void* stream);

/* tuning aid: force the workgroup tile ((64,64), (64,128), (128,128): the general small-tile kernel); bm = 0 restores the built-in
 * heuristic; bm = 1 / 3 forces the warp-specialised 128 x 128 / 64 x 128 tile (bn: ring, 0 = heuristic, 1 = 3 x 64-deep, (3,3) =
 * 3 x 128-deep), bm = 4 the eight-wave 256 x 128 ping-pong kernel, bm = 5 forbids it, bm = 9 the 256 x 256 kernel; (6, n) sets the ping-pong
 * kernel's minimum tile count, (7, 0|1) switches the grouped weight-gradient launch between the two kernel families, (11, 0|1) runs
 * the NT problems of the 256 x 128 kernel on v_mfma_f32_32x32x16_bf16 instead of 16x16x32, (12, n) = workgroups of nv_gemm_bf16_grouped_adamw (walking its
 * tiles; 0 = one per tile; default 128), (13, n) = at most n workgroups per nv_adamw_ranges launch (0 = one per 2048-element chunk) */
int nv_gemm_set_tile(int bm, int bn);

/* ---- LayerNorm folded into the GEMMs around it - inference forwards ("fused LayerNorm" as GEMM prologue; vit_3d.py:18-19,37-41):
 *   LN(x) W^T + b  =  rstd (x Wg^T) - rstd mu colsum(Wg) + (W beta + b),   Wg = W diag(gamma)
 * so a block's two LayerNorm launches (and their normalised copies) disappear: the GEMM that PRODUCES the residual stream (out-projection, FC2:
 * nv_gemm_resid_ln = nv_gemm_bf16 epilogue 4 without dropout) also writes the rows in the operand format and, per row and 128-column tile, (mean, sum of squared
 * deviations); the GEMM that CONSUMES them (to_qkv, FC1: nv_gemm_lnfold) contracts the un-normalised rows with Wg and applies mu / rstd - merged from the tile
 * partials by Chan's update, no E[x^2] - E[x]^2 - in its epilogue.  nv_ln_fold_weight prepares Wg (operand format), colsum (of the rounded Wg) and the folded bias.
 * Kernels with an LDS epilogue only (nv_gemm_lnfold_supported: every ViT3D-base shape from batch 1 up); same MFMA mainloops as nv_gemm_bf16. */
int nv_gemm_lnfold_supported(int M, int N, int K);
long nv_ln_fold_stats_floats(int M, int d);
int nv_ln_fold_weight(const float* W, long ldw, int N, int K, const float* gamma, const float* beta, const float* bias, void* Wg16, long ldg,
                      float* colsum, float* fbias, void* stream);
int nv_gemm_resid_ln(int M, int N, int K, const void* A, long lda, const void* W, long ldw, const float* bias, const float* resid, long ldr, float* out,
                     long ldo, void* out16, long ldo16, float* stats, void* stream);
int nv_gemm_lnfold(int gelu, int M, int N, int K, const void* X16, long ldx, const void* Wg16, long ldw, const float* stats, const float* colsum,
                   const float* fbias, float eps, void* out16, long ldo, void* stream);

/* ---- Linear layers on a few rows (the cls rows of the last block under pool='cls'): weight-streaming kernels, rows addressed through
 * leading dimensions (a [B, n, d] tensor's cls rows: ld = n * d).  bf16 operands, fp32 accumulation, cast points of nv_gemm_bf16.
 * nv_skinny_nt: W [N, K] row-major.  epi 0: out f32 [R, N] = resid + (bias + A W^T)   epi 1: u = bias + A W^T (bf16, optional), out bf16 = gelu(u)
 * nv_skinny_nn: W [K, N] row-major.  epi 0: out bf16 = (A W) * gelu'(u), dcol[n] (+)= column sums of the stored values (optional, R <= 4)
 *                                    epi 1: out f32 = A W     epi 2: out bf16 = A W */
/* (revision 5) drop_seed / drop_p: the nn.Dropout of the site (vit_3d.py:21,23,45), as in nv_gemm_bf16 - nt epi 0 on (bias + A W^T), epi 1 on gelu(u),
 * nn epi 0 on A W (the mask of the GELU output the gradient flows back through).  The mask is the one of the DENSE [M, N] tensor `out` is a
 * row-strided view of (ldo a multiple of N): element (r, n) of the view hashes at its offset r * ldo + n. */
int nv_skinny_nt(int epi, int R, int N, int K, const void* A, long lda, const void* W, long ldw, const float* bias, const float* resid,
                 long ldr, void* out, long ldo, void* u_out, long ldu, unsigned long drop_seed, float drop_p, void* stream);
int nv_skinny_nn(int epi, int R, int N, int K, const void* A, long lda, const void* W, long ldw, const void* u, long ldu, void* out, long ldo,
                 float* dcol, int accumulate, unsigned long drop_seed, float drop_p, void* stream);
/* out bf16 [total_rows, N] dense = zeros, except rows r * keep_every (r < R) = A[r, :] W: one launch (dAO of the last block under
 * pool = 'cls', whose incoming gradient lives on the cls rows only - clearing the other rows used to be a memset node) */
int nv_skinny_nn_sparse(int R, int N, int K, const void* A, long lda, const void* W, long ldw, void* out, long total_rows, int keep_every,
                        void* stream);

/* ---- LayerNorm of the residual stream (vit_3d.py:18,37): x f32 [M,d] -> y bf16, saves mean / rstd */
int nv_ln_fwd(const float* x, long ldx, int M, int d, const float* gamma, const float* beta, float eps, void* y, long ldy,
              float* mean, float* rstd, void* stream);
long nv_ln_bwd_workspace_bytes(int M, int d);
/* g_out = g_in + dLN(dy); g16 = bf16(g_out * mask); dgamma / dbeta / dcolsum(= column sums of g_out * mask) optional.
 * mask = the dropout mask (drop_seed, drop_p) of the Linear output that was added to this residual stream (1 if p = 0). */
int nv_ln_bwd(const float* dy, long lddy, const float* x, long ldx, const float* mean, const float* rstd, const float* gamma,
              int M, int d, const float* g_in, float* g_out, long ldg, void* g16, long ldg16, float* dgamma, float* dbeta,
              float* dcolsum, int accumulate, void* workspace, long ws_bytes, unsigned long drop_seed, float drop_p,
              void* stream, void* reduce_stream);
/* reduce_stream (null = stream): where the dgamma / dbeta / dcolsum reduction of the per-workgroup partials runs; it is
 * ordered after the main kernel by an event, and `workspace` must stay untouched until that stream has executed it.
 * NV_LN_NO_REDUCE leaves the reduction to a later nv_ln_bwd_reduce (same M, d, workspace) on a stream the caller has
 * ordered after this call - lets several reductions share one cross-stream event. */
#define NV_LN_NO_REDUCE ((void*)(-1L))
int nv_ln_bwd_reduce(const void* workspace, int M, int d, float* dgamma, float* dbeta, float* dcolsum, int accumulate, void* stream);

/* Several reductions of per-workgroup partial sums in ONE launch: out[s][c] (+)= sum_r partials[r][s * width + c].  A layer's bias
 * and LayerNorm-affine gradients (nv_ln_bwd with NV_LN_NO_REDUCE: rows = nv_ln_bwd_partial_rows(M), nseg = 3, width = d;
 * nv_gemm_bf16 epilogue 6: rows = ceil(M / nv_gemm_tile_rows), nseg = 1, width = N) all become final at the same point of the
 * backward pass; one launch instead of one per tensor.  count <= 8.  Deterministic (fixed summation order). */
typedef struct nv_reduce_job {
  const float* partials;
  int rows, width, nseg;
  float* out[3];           /* NULL = segment skipped */
  int accumulate;
} nv_reduce_job;
int nv_reduce_multi(const nv_reduce_job* jobs, int count, void* stream);
int nv_ln_bwd_partial_rows(int M);

/* ---- input contract (src/data/DatasetADNI.py:212-213, DatasetADNI_4D.py:86-87): crop of the raw volume + z-score
 * (x - mean) / (std + eps), population std over the whole cropped sample, statistics accumulated in double.
 * raw [B,X,Y,Z,T] with element strides (T = 1 for 3D), dtype 0 = float32 / 1 = int16; crop8 = {x0,y0,z0,t0,Sx,Sy,Sz,St};
 * out dense float32 [B,Sx,Sy,Sz,St]; stats (optional) [B,2] = mean, std. */
long nv_zscore_crop_workspace_bytes(int B);
/* statistics only: sigma[b] = population std of cropped volume b + eps, mean[b] optional (workspace as nv_zscore_crop) */
int nv_volume_sigma(const void* raw, int dtype, const long* strides5, int B, const int* crop8, float eps, float* sigma, float* mean,
                    void* workspace, long ws_bytes, void* stream);
int nv_zscore_crop(const void* raw, int dtype, const long* strides5, int B, const int* crop8, float eps, float* out,
                   float* stats, void* workspace, long ws_bytes, void* stream);

/* ---- patch embedding front end (vit_3d.py:92-93 + the permute of NeuroEncoder.py:200-202)
 * video [B,C,F,H,W] f32 with arbitrary element strides (pass the strides of the permuted VIEW of the
 * [B,H,W,D] dataset tensor - no copy); out bf16 [B*N, ldo] = LayerNorm(patch_dim)(patches).
 * Columns patch_dim .. ldo-1 of every row: nv_patch_ln_fwd and nv_patch_ln_fwd_f32 WRITE THEM AS ZERO (the padded K of the patch-embedding GEMM);
 * nv_patch_ln_fwd_4d and nv_patch_ln_fwd_4d_f32 leave them as they were.  No form writes a row it does not own. */
int nv_patch_ln_fwd(const float* video, const long* strides5, int B, int C, int F, int H, int W, int p1, int p2, int pf,
                    const float* gamma, const float* beta, float eps, void* out, long ldo, float* mean, float* rstd,
                    const float* vol_sigma, void* stream);
/* Two forms of the same arithmetic (bit-identical rows): a wave per token gathering its 64-byte runs itself (default: measured 14.5 us at
 * ViT3D-base batch 4), or a workgroup per patch COLUMN that stages its p1 * p2 rows of F contiguous floats through LDS with fully
 * coalesced reads and serves its F / pf tokens from there (frame stride 1, channels 1, the slab within 156 KiB of LDS - what a [B, H, W, D]
 * volume gives; 21 us: load, then compute, one workgroup per CU).  nv_patch_set_mode: 0 = the first, 2 = the second where it applies. */
int nv_patch_set_mode(int mode);
/* vol_sigma (may be NULL): [B] = std + 1e-8 of each RAW volume (nv_volume_sigma).  `video` is then the un-normalised (cropped
 * view of the) scanner volume: LayerNorm over a patch of (x - mu) / sigma equals LayerNorm over the patch of x with eps * sigma^2,
 * so the dataset's z-score (src/data/DatasetADNI.py:213) is folded into this kernel's epsilon - no normalised copy is written.
 * nv_patch_ln_fwd_4d: all T timepoints of a 4D sample x [Bo, H, W, D, T] (contiguous, T % 4 == 0; src/data/DatasetADNI_4D.py:86-96)
 * in one pass - replaces the strided regroup copy of NeuroEncoder.py:54-56; token rows (bo*T + t)*N + n. */
int nv_patch_ln_fwd_4d(const float* x, int Bo, int H, int W, int D, int T, int p1, int p2, int pf, const float* gamma,
                       const float* beta, float eps, void* out, long ldo, float* mean, float* rstd, const float* vol_sigma,
                       void* stream);
/* fp32 tokens (fp32 inference path): out f32 [B*N, ldo], ldo >= patch_dim */
int nv_patch_ln_fwd_f32(const float* video, const long* strides5, int B, int C, int F, int H, int W, int p1, int p2, int pf,
                        const float* gamma, const float* beta, float eps, float* out, long ldo, float* mean, float* rstd,
                        const float* vol_sigma, void* stream);
int nv_patch_ln_fwd_4d_f32(const float* x, int Bo, int H, int W, int D, int T, int p1, int p2, int pf, const float* gamma,
                           const float* beta, float eps, float* out, long ldo, float* mean, float* rstd, const float* vol_sigma,
                           void* stream);
long nv_patch_ln_bwd_workspace_bytes(int tokens, int P);
int nv_patch_ln_bwd(const float* video, const long* strides5, int B, int C, int F, int H, int W, int p1, int p2, int pf,
                    const float* dxp, long ldd, const float* mean, const float* rstd, float* dgamma, float* dbeta,
                    int accumulate, void* workspace, long ws_bytes, void* stream);
/* (revision 7) backward of LayerNorm(patch_dim) w.r.t. its input, scattered back into voxel layout: dvideo (f32, geometry of `video`,
 * element strides dstrides5) = d loss / d video, from dxp [B*N, ldd] (the gradient at the LayerNorm's output; columns P .. ldd-1 are
 * not read), the forward's token statistics and gamma.  The volume is re-gathered (fp32).  Every element of dvideo is written exactly
 * once (the patches tile the volume): no clearing needed. */
int nv_patch_ln_dx(const float* video, const long* strides5, int B, int C, int F, int H, int W, int p1, int p2, int pf,
                   const float* dxp, long ldd, const float* mean, const float* rstd, const float* gamma,
                   float* dvideo, const long* dstrides5, void* stream);

/* ---- LayerNorm(dim) + cls token + positional embedding (vit_3d.py:95,116-118): t [B*N,d] -> x [B,N+1,d] */
int nv_embed_finish_fwd(const float* t, long ldt, int B, int N, int d, const float* gamma, const float* beta, float eps,
                        const float* pos, const float* cls, float* x, long ldx, float* mean, float* rstd,
                        unsigned long drop_seed, float drop_p, void* stream);
long nv_embed_finish_bwd_workspace_bytes(int B, int N, int d);
/* dgamma, dbeta, dbias_pe, dpos, dcls: all given, or (revision 7) all NULL - then only dt / dt16 are produced (data-only backward) */
int nv_embed_finish_bwd(const float* g, long ldg, const float* t, long ldt, const float* mean, const float* rstd,
                        const float* gamma, int B, int N, int d, float* dt, long lddt, void* dt16, long lddt16, float* dgamma,
                        float* dbeta, float* dbias_pe, float* dpos, float* dcls, int accumulate, void* workspace, long ws_bytes,
                        unsigned long drop_seed, float drop_p, void* stream);

/* ---- multi-head attention core (vit_3d.py:51-59): qkv bf16 [B,n,3*inner] -> out bf16 [B,n,inner], lse f32 [B,heads,n] */
int nv_attn_set_mode(int mode);   /* testing aid: 0 = heuristic, 1 = streaming kernels, 2 = LDS-resident kernels (n <= 576), 3 = wide streaming forward;
                                    + 20: resident forward with two partner waves per row group (key range split, merged through LDS);
                                    + 100: resident backward as ONE launch whose dK / dV workgroups compute delta themselves, instead of two
                                    dependent launches (dQ, then dK / dV reading its delta): same results bit for bit, measured slower */
int nv_attn_fwd(const void* qkv, long ld_qkv, int B, int n, int heads, int dim_head, float scale, void* out, long ld_out,
                float* lse, unsigned long drop_seed, float drop_p, void* stream);
/* the same forward with the output as OCP e4m3 bytes of (value * out_scale): out = byte buffer [B*n, ld_out]; dim_head 64, no dropout, no lse */
int nv_attn_fwd_o8(const void* qkv, long ld_qkv, int B, int n, int heads, int dim_head, float scale, void* out, long ld_out,
                   float out_scale, void* stream);
int nv_attn_bwd(const void* qkv, long ld_qkv, const void* out, const void* dout, long ld_out, const float* lse, int B, int n,
                int heads, int dim_head, float scale, float* delta, void* dqkv, long ld_dqkv, unsigned long drop_seed,
                float drop_p, void* stream);
/* (revision 8) attention probabilities P = softmax(scale q k^T) of one layer, recomputed from its qkv - the output of the reference's
 * `attend` (vit_3d.py:54) in its 'b h n d' head order.  qkv_f32 = 0: qkv in the 16-bit operand format (as nv_attn_fwd; dim_head a
 * multiple of 8 up to 128), 1: fp32 (as nv_attn_fwd_f32; a multiple of 4 up to 128).  Row statistics are computed here from q and k
 * (no lse needed).  out fp32, contiguous:
 *   fusion NV_ATTN_PER_HEAD: [B, heads, R, n];  NV_ATTN_FUSE_MEAN / _MAX / _MIN: [B, R, n] = mean / max / min over the heads, one launch
 *   rows NV_ATTN_ROWS_ALL: R = n;  NV_ATTN_ROWS_CLS: R = 1 (row 0, the cls token's)
 * A probability has the same bits in every form (max / min fusion = the reduction of the per-head output, exactly). */
#define NV_ATTN_PER_HEAD 0
#define NV_ATTN_FUSE_MEAN 1
#define NV_ATTN_FUSE_MAX 2
#define NV_ATTN_FUSE_MIN 3
#define NV_ATTN_ROWS_ALL 0
#define NV_ATTN_ROWS_CLS 1
int nv_attn_probs(int qkv_f32, const void* qkv, long ld_qkv, int B, int n, int heads, int dim_head, float scale, int fusion, int rows,
                  float* out, void* stream);
/* (revision 8) attention rollout: out [B, n - 1] = the patch-token entries (token order) of u A^_{L-1} ... A^_0 with
 * A^_l = (A_l + I) / (rowsum(A_l) + 1) row-wise - the head-fused (A + I) / 2, row-renormalised rule, exact also for max / min fusion.
 * maps: HOST array [L] of device pointers to head-fused all-rows maps [B, n, n] (nv_attn_probs).  u = e_0 (the cls row) or, with
 * start_mean = 1, the mean of all rows (pool = 'mean').  Two memory-bound launches per layer; workspace nv_attn_rollout_workspace_bytes. */
long nv_attn_rollout_workspace_bytes(int B, int n);
int nv_attn_rollout(const float* const* maps, int L, int B, int n, int start_mean, float* out, void* workspace, long ws_bytes, void* stream);
/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) gradient of the loss w.r.t. the attention
 * probabilities of one layer, recomputed behind its attention backward from the layer's qkv (operand format, as nv_attn_probs with
 * qkv_f32 = 0; dim_head a multiple of 8 up to 128) and dout = the 16-bit gradient of the attention output [B * n, ld_dout] (what
 * nv_attn_bwd takes).  What a backward hook on the reference's `attend` (vit_3d.py:54), or attn.register_hook, delivers.  out fp32, contiguous:
 *   form NV_ATTN_GRAD_PER_HEAD:  [B, heads, n, n] = dO_h V_h^T, the reference's 'b h n d' head order; no probabilities involved;
 *   form NV_ATTN_GRAD_RELEVANCE: [B, n, n] = (1 / heads) sum_h max(dP_h * P_h, 0) - the layer term of gradient-weighted attention
 *     relevance (Chefer et al., "Generic Attention-model Explainability"); P_h has the bits of the nv_attn_probs export.
 * Both products run on the 16x16x32 MFMA with fp32 accumulation.  Rows of dout that are exact zeros give exact zero rows.  No dropout:
 * the gradient is the one w.r.t. the output of `attend`, in front of the attention dropout, of a forward that had none. */
#define NV_ATTN_GRAD_PER_HEAD 0
#define NV_ATTN_GRAD_RELEVANCE 1
int nv_attn_grad(const void* qkv, long ld_qkv, const void* dout, long ld_dout, int B, int n, int heads, int dim_head, float scale, int form,
                 float* out, void* stream);
/* class-specific token relevance: out [B, n - 1] = the patch-token entries (token order) of u (I + A_{L-1}) ... (I + A_0), evaluated as
 * u <- u + u A_l from the last layer down - the row of R <- R + A_l R (R = I at the start, first layer first) that belongs to the token
 * the head reads.  maps: HOST array [L] of device pointers to relevance-form maps [B, n, n] (nv_attn_grad).  u = e_0 (the cls row) or,
 * with start_mean = 1, the mean of all rows (pool = 'mean').  No renormalisation.  One memory-bound launch per layer. */
long nv_attn_relevance_workspace_bytes(int B, int n);
int nv_attn_relevance(const float* const* maps, int L, int B, int n, int start_mean, float* out, void* workspace, long ws_bytes, void* stream);
int nv_stream_sync(void* from, void* to);   /* stream `to` waits for everything enqueued so far on `from` (pooled events) */
int nv_spin_us(int microseconds, void* stream);   /* one wave that keeps `stream` busy for the given time (<= 50 ms): stream-placement probes */

/* ---- classification head (vit_3d.py:107-110,123-126): cls row -> LayerNorm -> Linear(dim, C), fp32 */
int nv_head_fwd(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps,
                const float* W, const float* bias, int C, float* xh, float* stats, float* logits, void* stream);
long nv_head_bwd_workspace_bytes(int B, int d);
/* dgamma, dbeta, dW, dbias: all given (dcolsum may be NULL), or (revision 7) all five NULL - then only g / g16 are produced */
int nv_head_bwd(const float* dlogits, int B, int C, const float* W, const float* x, long row_stride, const float* stats,
                const float* xh, const float* gamma, int d, int n, float* g, long ldg, void* g16, long ldg16, float* dgamma,
                float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                unsigned long drop_seed, float drop_p, int pool_mean, void* stream);
/* nv_head_fwd + nv_ce_loss + nv_head_bwd (pool = 'cls') in TWO launches instead of five, every output bit-identical to the three calls
 * (launch 1: one workgroup per volume runs the bodies of their per-volume kernels back to back, the other workgroups clear g / g16
 * outside the cls rows; launch 2: every sum over the volumes): mlp_head forward, nn.CrossEntropyLoss (mean) and their backward,
 * vit_3d.py:118-123,128-130 + Trainer.py:70,74.  workspace: nv_head_step_workspace_bytes(B, d). */
long nv_head_step_workspace_bytes(int B, int d);
int nv_head_step(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps, const float* W,
                 const float* bias, int C, const long* labels, float grad_scale, float* xh, float* stats, float* logits, float* loss,
                 float* dlogits, int n, float* g, long ldg, void* g16, long ldg16, float* dgamma, float* dbeta, float* dW, float* dbias,
                 float* dcolsum, int accumulate, void* workspace, long ws_bytes, unsigned long drop_seed, float drop_p, void* stream);
/* pool='mean' (vit_3d.py:127): out[b,:] = mean_t x[b,t,:]; feed it to nv_head_fwd / nv_head_bwd with row_stride = d
   and pool_mean = 1 (every row of g then receives dx / n) */
int nv_token_mean(const float* x, int B, int n, int d, float* out, void* stream);

/* ---- bias gradients: out[c] (+)= sum_r X[r,c], X bf16 */
long nv_colsum_workspace_bytes(int M, int N);
int nv_colsum_bf16(const void* X, long ld, int M, int N, float* out, int accumulate, void* workspace, long ws_bytes,
                   void* stream);

/* ---- loss / optimizer (Trainer.py:30-31,70,75): nn.CrossEntropyLoss (mean) and torch.optim.AdamW */
int nv_ce_loss(const float* logits, const long* target, int B, int C, float grad_scale, float* loss, float* dlogits,
               void* stream);
int nv_adamw_step(float* p, const void* grad, int grad_bf16, float* m, float* v, void* p16, long count, int step, double lr,
                  double beta1, double beta2, double eps, double weight_decay, float grad_scale, int max_blocks, void* stream);
/* ---- dynamic loss scale for NV_OPERAND_FP16 training: torch.amp.GradScaler (src/Trainer.py:29,74-76) kept on the device - no
 * found_inf read-back per step.  `state`: NV_LOSS_SCALE_FLOATS floats of device memory owned by the caller; [0] = current scale,
 * [5] = optimizer updates applied so far, [11] = updates skipped (the rest: common.h LS_*).  Per optimizer step:
 *   nv_ce_loss_scaled / nv_head_step_scaled   d(loss)/d(logits) is multiplied by state[0] (the reported loss is not)
 *   nv_loss_scale_check(grads, count, state)  found_inf |= any inf / NaN in grads[0 .. count)   (after the backward pass / all-reduce)
 *   nv_loss_scale_update(state, lr, b1, b2)   decides skip or step: backoff / growth of the scale, AdamW's step count and bias
 *                                             corrections (double arithmetic, as torch forms them), 1 / scale for the update
 *   nv_adamw_step_scaled(..., state, stream)  nv_adamw_step that does nothing when the step is skipped and un-scales the gradients
 *                                             (its `step` argument is ignored: the state's own count of applied updates is used)
 * GradScaler defaults: init_scale 65536, growth_factor 2, backoff_factor 0.5, growth_interval 2000.  start_step = updates already
 * applied to the optimizer state. */
#define NV_LOSS_SCALE_FLOATS 16
int nv_loss_scale_init(float* state, float init_scale, float growth_factor, float backoff_factor, int growth_interval, int start_step, void* stream);
int nv_loss_scale_check(const float* grads, long count, float* state, void* stream);
int nv_loss_scale_update(float* state, double lr, double beta1, double beta2, void* stream);
int nv_ce_loss_scaled(const float* logits, const long* target, int B, int C, float grad_scale, const float* scale_state, float* loss,
                      float* dlogits, void* stream);
int nv_adamw_step_scaled(float* p, const void* grad, int grad_bf16, float* m, float* v, void* p16, long count, int step, double lr,
                         double beta1, double beta2, double eps, double weight_decay, float grad_scale, int max_blocks,
                         const float* scale_state, void* stream);
int nv_head_step_scaled(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps, const float* W,
                        const float* bias, int C, const long* labels, float grad_scale, const float* scale_state, float* xh, float* stats,
                        float* logits, float* loss, float* dlogits, int n, float* g, long ldg, void* g16, long ldg16, float* dgamma,
                        float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                        unsigned long drop_seed, float drop_p, void* stream);
/* ---- global-norm gradient clipping on the device: scaler.unscale_(opt); torch.nn.utils.clip_grad_norm_(params, max_norm); scaler.step(opt)
 * with the norm never read by the host.  `clip_state`: NV_GRAD_CLIP_BYTES of device memory owned by the caller, 8-byte aligned and
 * ZEROED once before the first use.  As floats: [0..1] = one double, the running sum of squares; [2] = total_norm and [3] = coef of
 * the last finished step; [4..15] reserved; from [16] on NV_GRAD_CLIP_MAX_BLOCKS doubles, one partial per workgroup (common.h GC_*).
 * Per optimizer step:
 *   nv_grad_sumsq(grad, is16, count, clip_state, scale_state, max_blocks)   once per gradient buffer (arena, 16-bit reduced message
 *                        buffer, stock tensor; any count >= 1, element-aligned): running sum += sum x^2, every element widened to
 *                        double first - finite fp32 gradients always give a finite sum, and bits reproduce from run to run (no
 *                        atomics).  scale_state (may be NULL): found_inf is raised when the sum is not finite, so with a dynamic
 *                        loss scale this pass REPLACES nv_loss_scale_check.  max_blocks > 0 caps the grid.
 *   nv_loss_scale_update (only with a dynamic loss scale) - before the next call, which reads the 1 / scale it writes
 *   nv_grad_clip_finish(clip_state, max_norm, grad_scale, scale_state)      total_norm = sqrt(sum) * |grad_scale| * (scale_state ?
 *                        1 / scale : 1) as fp32;  coef = min(max_norm / (total_norm + 1e-6), 1) in fp32 as clip_grad_norm_ forms it
 *                        (infinite norm: 0, NaN norm: NaN, exactly 1 when the bound does not bind);  running sum = 0
 *   nv_adamw_step_clipped(..., scale_state, clip_state, stream)             nv_adamw_step_scaled (scale_state may be NULL) whose
 *                        gradient factor is also multiplied by coef.  The gradients themselves are left as they are. */
#define NV_GRAD_CLIP_MAX_BLOCKS 2048
#define NV_GRAD_CLIP_BYTES (64 + 8 * NV_GRAD_CLIP_MAX_BLOCKS)
int nv_grad_sumsq(const void* grad, int grad_16bit, long count, float* clip_state, float* scale_state, int max_blocks, void* stream);
int nv_grad_clip_finish(float* clip_state, float max_norm, float grad_scale, const float* scale_state, void* stream);
int nv_adamw_step_clipped(float* p, const void* grad, int grad_bf16, float* m, float* v, void* p16, long count, int step, double lr,
                          double beta1, double beta2, double eps, double weight_decay, float grad_scale, int max_blocks,
                          const float* scale_state, const float* clip_state, void* stream);
/* grad_bf16 = 1: `grad` is a bf16 buffer (the gradient all-reduce ran on bf16 messages): no cast back to fp32 is needed. */
/* max_blocks > 0 caps the grid (256-thread workgroups, grid-stride): used when the update of one gradient bucket runs on a
   side stream beside the backward pass, so that it takes a slice of the chip instead of queueing ahead of the GEMMs. */
/* ---- parameter groups for the fused AdamW (neurovit_amd.FusedAdamW with more than one (lr, weight_decay); added within revision 8):
 * nv_adamw_step_clipped over the flat arena [0, count) - the same pointers, fp32 or 16-bit gradients, optional 16-bit shadow in the
 * current operand format, grad_scale, max_blocks, optional scale_state and clip_state - whose lr and weight_decay come from a table.
 *   groups    G of them, 1 <= G <= NV_ADAMW_MAX_GROUPS, each with its own lr_g and weight_decay_g (finite, >= 0); beta1, beta2 and eps
 *             are shared.  They travel with every call, in nv_adamw_groups: decay_g = float(1 - lr_g * weight_decay_g) and
 *             step_size_g = float(lr_g / (1 - beta1^step)) are formed in double per call, as nv_adamw_step forms its own, and reach
 *             the kernel as arguments - no copy, no synchronisation.  With scale_state the step count is the device block's: a
 *             one-wave launch in front forms step_size_g from it with the expression of nv_loss_scale_update (`step` is ignored and
 *             the block's own step size, formed from the lr that nv_loss_scale_update got, is not read).
 *   segments  S of them, 1 <= S <= NV_ADAMW_MAX_SEGMENTS: segment s covers the elements [end[s-1], end[s]) (end[-1] = 0) and belongs
 *             to group group[s].  Ends ascend strictly, the last is `count`; a boundary may fall at ANY element.  The table is static
 *             for a model and lives in device memory that the caller owns: nv_adamw_segments_bytes(S) bytes, 16-byte aligned, filled
 *             ONCE by nv_adamw_segments_build, which checks the host arrays (NV_ERR_ARG: S or G out of range, ends not ascending, last
 *             end != count, a group index >= G, count no positive multiple of 4, a table too small), uploads them and returns when the
 *             copy has finished (not inside a stream capture).  The library remembers the addresses it has built:
 *             nv_adamw_step_grouped refuses a table it did not build, or one built for another G or count.  Call
 *             nv_adamw_segments_release before freeing the memory (the address is forgotten; building again over it is also fine).
 *             The tail of the buffer is scratch of the step under a scale_state: one table serves one stream at a time.
 * Every element gets the bits nv_adamw_step_clipped gives it when called with its own group's lr and weight_decay.
 * nv_adamw_step_grouped returns NV_ERR_ARG before any launch for: a null p / grad / m / v or the alignments nv_adamw_step asks for,
 * count no positive multiple of 4, step < 1, a wrong struct_size, G out of range, a non-finite or negative lr_g / weight_decay_g,
 * a segment table that was not built, or was built for another G or count. */
#define NV_ADAMW_MAX_GROUPS 64
#define NV_ADAMW_MAX_SEGMENTS 1024
typedef struct nv_adamw_groups {
  int struct_size;                              /* sizeof(nv_adamw_groups) */
  int n_groups;                                 /* G */
  const void* segments;                         /* device table filled by nv_adamw_segments_build */
  double lr[NV_ADAMW_MAX_GROUPS];               /* [0, G) are read */
  double weight_decay[NV_ADAMW_MAX_GROUPS];
} nv_adamw_groups;
long nv_adamw_segments_bytes(int segments);     /* 0 for a count outside 1 .. NV_ADAMW_MAX_SEGMENTS */
int nv_adamw_segments_build(void* table, long table_bytes, const long* ends, const int* groups, int segments, int n_groups, long count, void* stream);
int nv_adamw_segments_release(void* table);
int nv_adamw_step_grouped(float* p, const void* grad, int grad_bf16, float* m, float* v, void* p16, long count, int step,
                          const nv_adamw_groups* groups, double beta1, double beta2, double eps, float grad_scale, int max_blocks,
                          const float* scale_state, const float* clip_state, void* stream);
/* ---- exponential moving average of a parameter arena (neurovit_amd.ModelEma; added within revision 8):
 *   ema[i] = ema[i] + (p[i] - ema[i]) * weight     for i in [0, count)
 * in fp32, the difference, the product and the sum each rounded on their own (no fused multiply-add): bit-equal to the same torch
 * expression on the CPU, and p[i] == ema[i] leaves ema[i] unchanged bit for bit (inf / NaN propagate as in that expression).
 * weight = float32(1 - decay) is formed by the caller; 0 <= weight <= 1, NaN is refused.  count > 0 and a multiple of 4 (arena
 * segments are padded); both pointers 16-byte aligned; p is only read; no 16-bit shadow of ema is written.  max_blocks as above. */
int nv_ema_update(float* ema, const float* p, long count, float weight, int max_blocks, void* stream);
int nv_cast_bf16_2d(const float* src, long ld_src, int rows, int cols, void* dst, long ld_dst, void* stream);
/* out16 (bf16) / out32 (f32), either may be NULL: x[M,N] f32 times the nn.Dropout mask of one site (same mask as the GEMM
 * epilogues, element index m*N + n; drop_p = 0: plain cast / copy).  Standalone Attention / FeedForward modules (vit_3d.py:23,45). */
int nv_dropout_apply(const float* x, long ldx, int M, int N, unsigned long drop_seed, float drop_p, void* out16, long ld16,
                     float* out32, long ld32, void* stream);
int nv_copy_2d_f32(const float* src, long ld_src, int rows, int cols, float* dst, long ld_dst, int accumulate, void* stream);

/* ---- Grad-CAM reduction (src/models/NeuroEncoder.py:101-116): act bf16 [B,n,d] = output of the last block's attention
 * LayerNorm, grad f32 [B,n,d] = its gradient -> cam f32 [B, n-1]: relu(mean_d(grad) * sum_d(act)) of the patch tokens
 * (cls dropped), min-max normalised over the whole map ((x - min) / (max - min + 1e-8)); minmax (optional) [2] = the raw
 * min / max.  One launch; the percentile threshold and the trilinear upsampling of the G^3 map stay with the caller. */
long nv_gradcam_workspace_bytes(int B, int n);
int nv_gradcam_reduce(const void* act, const float* grad, int B, int n, int d, float* cam, float* minmax, void* workspace,
                      long ws_bytes, void* stream);
/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) batched attribution volumes: every volume of the
 * batch on its own, nothing leaves the device.
 * nv_gradcam_reduce_per_volume: nv_gradcam_reduce with the min-max normalisation taken over each volume's own n - 1 cells; minmax
 * (optional) [B, 2].  Volume b has the bits of nv_gradcam_reduce called with B = 1 on that volume's slice.  One launch.
 * nv_token_map_to_volume: maps [B, G0 G1 G2] (token order, reshaped as is: NeuroEncoder.py:117-131) -> out [B, S0, S1, S2] fp32.
 * grid3 / out3: HOST arrays {G0, G1, G2} / {S0, S1, S2}.  Per volume:
 *   normalize = 1: (v - min) * (1 / (max - min + 1e-8)) over the volume's cells (0: the map is taken as it is);
 *   cut = torch.quantile(cells.double(), 1 - keep_percent / 100, interpolation='linear') rounded to fp32: pos = q (N - 1), lo = floor(pos),
 *     hi = min(lo + 1, N - 1), w = pos - lo, cut = s[lo] + w (s[hi] - s[lo]) for w < 0.5, else s[hi] - (s[hi] - s[lo]) (1 - w), in double,
 *     s = the order statistics of the cells; cells >= cut are kept, the rest become 0 (keep_percent = 100 keeps everything);
 *   trilinear upsampling G -> S with align_corners = False and ATen's index arithmetic: per axis src = max((dst + 0.5) (G / S) - 0.5, 0)
 *     in fp32, i0 = floor(src), i1 = min(i0 + 1, G - 1), lambda1 = src - i0, lambda0 = 1 - lambda1.
 * Maps hold finite values.  G0 G1 G2 <= 4096 (16^3) and G1 G2 + 2 S1 + 2 S2 <= 16384, NV_ERR_ARG beyond; out and workspace 16-byte aligned.
 * Two launches: one workgroup per volume (selection in LDS), then a streaming kernel with 16-byte stores.  On return the workspace holds
 * [B, N] normalised maps, [B, N] thresholded maps, [B] cuts (fp32, in this order), which a caller may read. */
long nv_gradcam_per_volume_workspace_bytes(int B, int n);
int nv_gradcam_reduce_per_volume(const void* act, const float* grad, int B, int n, int d, float* cam, float* minmax, void* workspace,
                                 long ws_bytes, void* stream);
long nv_token_map_to_volume_workspace_bytes(int B, const int* grid3);
int nv_token_map_to_volume(const float* maps, int B, const int* grid3, const int* out3, int normalize, double keep_percent, float* out,
                           void* workspace, long ws_bytes, void* stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) perturbation attribution: the device steps around
 * the forward of deletion / insertion curves and of patch occlusion sensitivity.  No call allocates or synchronises; every argument
 * is checked first (NV_ERR_ARG).  `jobs` is a DEVICE array int32 [J, 3] of rows (b, lo, hi): b the source volume of the job.
 * nv_token_ranks: maps fp32 [B, N] (finite values, N <= 4096) -> ranks int32 [B, N],
 *     ranks[b, t] = #{ j : maps[b, j] > maps[b, t]  or  (maps[b, j] == maps[b, t] and j < t) }:
 *   descending order, ties to the lower token index, -0.0 == +0.0 a tie; a permutation of 0 .. N - 1 and the inverse of
 *   torch.sort(maps, descending=True, stable=True).indices.  One workgroup per volume, a counting pass over the keys in LDS.
 * nv_mask_patches: x fp32 [B, S0, S1, S2] dense (NeuroEncoder.forward's [B, H, W, D]), labels int32 [B, N], size3 / patch3 HOST arrays
 *   {S0, S1, S2} / {p0, p1, p2} (S_a a multiple of p_a, G_a = S_a / p_a, N = G0 G1 G2 <= 4096, N + S1 + S2 <= 16320)
 *   -> out fp32 [J, S0, S1, S2] (16-byte aligned).  Voxel (i0, i1, i2) belongs to token t = (i2 / p2) G0 G1 + (i0 / p0) G1 + i1 / p1 (the
 *   patchify order of the engine's gather, vit_3d.py:92 on the [B, 1, D, H, W] view).  For job j = (b, lo, hi):
 *     out[j, i0, i1, i2] = lo <= labels[b, t] < hi ? baseline : x[b, i0, i1, i2]
 *   with baseline = `value` (base NULL), or base[b * base_stride + (i0 S1 + i1) S2 + i2] (base_stride in elements; 0 = one volume shared
 *   by every job).  A pure select: every bit of x and of the baseline passes through (NaN, Inf, -0.0).  A job with b outside [0, B)
 *   reads nothing and writes nothing; lo >= hi copies x[b].  One launch, 16-byte stores whatever the alignment of the volumes (27^3).
 *   nv_mask_patches_set_group (A/B aid, process-wide, 1 .. 16, default 4): consecutive jobs one workgroup serves from one read of x.
 * nv_class_scores: logits fp32 [J, C], cls int64 [B] -> scores fp32 [J] of class c = cls[b_j]: NV_SCORE_LOGIT copies logits[j, c] bit for bit,
 *   NV_SCORE_PROB is exp(l_c - max) / sum_i exp(l_i - max) in fp32 with the library expf.  b_j outside [0, B): nothing written; c outside
 *   [0, C): NaN.
 * nv_curve_auc: scores fp32 [B, K] with row stride ld (elements), K >= 2 -> auc fp32 [B]: the trapezoid rule on the uniform grid k / (K - 1),
 *   (sum_k s_k - (s_0 + s_{K-1}) / 2) / (K - 1), summed in double in index order, stored as fp32.
 * nv_occlusion_gather: ref fp32 [B], scores fp32 [B, NB], labels int32 [B, N] -> maps fp32 [B, N] = ref[b] - scores[b, labels[b, t]]
 *   (a label outside [0, NB): NaN). */
#define NV_SCORE_PROB 0
#define NV_SCORE_LOGIT 1
int nv_token_ranks(const float* maps, int B, int N, int* ranks, void* stream);
int nv_mask_patches(const float* x, int B, const int* size3, const int* patch3, const int* labels, const int* jobs, int J, float value,
                    const float* base, long base_stride, float* out, void* stream);
int nv_mask_patches_set_group(int group);
int nv_class_scores(const float* logits, int J, int C, const int* jobs, const long* cls, int B, int kind, float* scores, void* stream);
int nv_curve_auc(const float* scores, int B, int K, long ld, float* auc, void* stream);
int nv_occlusion_gather(const float* ref, const float* scores, const int* labels, int B, int N, int NB, float* maps, void* stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) Shapley value sampling over players on the patch
 * grid (patch tokens, blocks of them, atlas regions): the device steps around the forward.  No call allocates, synchronises or reads
 * anything back; every argument is checked first (NV_ERR_ARG).  No atomics: every output cell is owned by one thread and two runs give
 * the same bits.  Every double operation is rounded on its own (no FMA contraction).
 * nv_mask_patches_rows: nv_mask_patches (the same kernel body, token rule, baseline forms and 16-byte stores at any alignment) with
 *   labels int32 [Rows, N] and jobs int32 [J, 4] of rows (b, row, lo, hi):
 *     out[j, i0, i1, i2] = lo <= labels[row, t] < hi ? baseline : x[b, i0, i1, i2]
 *   A job with b outside [0, B) or row outside [0, Rows) reads nothing and writes nothing; lo >= hi copies x[b].  Consecutive jobs of
 *   one volume and one row share one read of x and of the labels.
 * nv_shapley_ranks: writes ranks int32 [U R, B, F] (DEVICE), 2 <= F <= 4096 players, R = 1 or 2, U <= 65535 units per call.  For unit u,
 *   sample b, player f:
 *     seed_s = nv_hash64(seed, 0x53484150)     (a domain of its own: no dropout, augmentation, mix, affine, MIM or drop-path draw is reused)
 *     h      = nv_hash64(seed_s, (((first_unit + u) 2^32 + b) 4096 + f) mod 2^64)
 *     key_f  = (h >> 40) 2^-24 (exact in fp32);  rank_f = #{ j : key_j > key_f or (key_j == key_f and j < f) }   (nv_token_ranks' rule)
 *   Row r = 0 of unit u (ranks[(u R + r), b, :]) holds rank, a permutation of 0 .. F - 1; with R = 2, row r = 1 holds the antithetic
 *   permutation F - 1 - rank.  first_unit + U <= 2^32.  One workgroup per (unit, sample), the keys ranked in LDS.
 * nv_shapley_labels: ranks int32 [Rows, F], features int32 [B, N] -> labels int32 [Rows, N]; row q belongs to volume q mod B:
 *     labels[q, t] = ranks[q, features[q mod B, t]];   a feature id outside [0, F) (the convention is -1) gives label F: such a patch
 *   is no player, and a job (b, row, k, F) leaves it as in x.
 * nv_shapley_accumulate: interior fp32 [U R, B, F - 1], ends fp32 [B, 2], ranks int32 [U R, B, F] -> values fp32 [B, F], std_err fp32
 *   [B, F], delta fp32 [B], sums double [B, F, 2].  The score row of permutation q = u R + r of volume b is s_0 = ends[b, 0] (nothing
 *   present), s_k = interior[q, b, k - 1] for 0 < k < F (the k first-ranked players present), s_F = ends[b, 1].  Player f of rank rho has
 *   the marginal m = double(s_{rho+1}) - double(s_rho); a unit's value v_u is m (R = 1) or (m_0 + m_1) / 2 (R = 2).  In unit order,
 *     sums[b, f, 0] = sum_u v_u,  sums[b, f, 1] = sum_u v_u v_u;   values = fp32(sum / U);
 *     std_err = fp32(sqrt(max((sumsq - sum sum / U) / (U - 1), 0) / U)),  NaN for U = 1;
 *     delta[b] = fp32((sum_f sums[b, f, 0]) / U - (double(s_F) - double(s_0))),  the sum in player order: the efficiency residual.
 *   A rank outside [0, F) is clamped (no read outside the row).  One thread owns (b, f).
 * nv_shapley_token_maps: values fp32 [B, F], features int32 [B, N] (F, N <= 4096) -> maps fp32 [B, N]: a patch of player f gets
 *   values[b, f] / (number of patches of f in volume b) (one fp32 division), a patch of no player 0: the map sums to the values. */
int nv_mask_patches_rows(const float* x, int B, const int* size3, const int* patch3, const int* labels, int Rows, const int* jobs, int J,
                         float value, const float* base, long base_stride, float* out, void* stream);
int nv_shapley_ranks(unsigned long seed, unsigned long first_unit, int U, int R, int B, int F, int* ranks, void* stream);
int nv_shapley_labels(const int* ranks, const int* features, int Rows, int B, int F, int N, int* labels, void* stream);
int nv_shapley_accumulate(const float* interior, const float* ends, const int* ranks, int U, int R, int B, int F, float* values, float* std_err,
                          float* delta, double* sums, void* stream);
int nv_shapley_token_maps(const float* values, const int* features, int B, int F, int N, float* maps, void* stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) path attribution: the device steps around the
 * forward and the data-only backward of integrated gradients.  No call allocates or synchronises; every argument is checked first
 * (NV_ERR_ARG).  `jobs` is a DEVICE array int32 [J, 2] of rows (b, k): b the source volume of the job, k its step on the path.
 * The first four see a sample as V dense floats (no geometry); rows of a [rows, V] buffer may start at any 4-byte alignment (27^3), the
 * buffer each call WRITES is 16-byte aligned.  Every sum and product below is one separately rounded fp32 operation (round to nearest
 * even, no FMA), so the results are the bits of the same expressions evaluated as separate torch tensor operations on the CPU.  No
 * atomics: every output element is owned by one thread, and two runs give the same bits.
 * nv_path_points: x fp32 [B, V], alphas fp32 [K] -> out fp32 [J, V].  For job j = (b, k):
 *     out[j, e] = bl + alphas[k] * (x[b, e] - bl)
 *   with bl = `value` (base NULL), or base[b * base_stride + e] (base_stride in elements; 0 = one volume shared by every job).  NaN and
 *   Inf propagate as the three operations propagate them.  A job with b outside [0, B) or k outside [0, K) reads nothing and writes
 *   nothing.  One launch; consecutive jobs of one volume are served from one read of x and of the baseline.
 * nv_class_score_grads: logits fp32 [J, C], cls int64 [B] -> dlogits fp32 [J, C], the gradient of the score of class c = cls[b_j] w.r.t.
 *   row j: NV_SCORE_LOGIT the one-hot of c; NV_SCORE_PROB p_c (delta_ci - p_i) with p the fp32 softmax of nv_class_scores (max-subtracted,
 *   the library expf).  b_j outside [0, B): nothing written; c outside [0, C): a row of NaN.
 * nv_path_accumulate: g fp32 [J, V], weights fp32 [K], acc fp32 [B, V].  For every volume b that appears in `jobs` (with k in [0, K)):
 *     acc[b] <- (..((acc[b] + w_k1 * g[j1]) + w_k2 * g[j2]) ..)   over that volume's jobs j1 < j2 < .. in job order.
 *   The call always adds: the caller zero-fills acc once, on the same stream.  Volumes absent from `jobs` are not touched.  J <= 1024.
 * nv_path_finish: attr[b, e] = (x[b, e] - bl) * acc[b, e]   (x, acc, attr fp32 [B, V]; the baseline as nv_path_points).
 * nv_attr_token_sums: attr fp32 [B, S0, S1, S2] dense, size3 / patch3 HOST arrays and the token rule of nv_mask_patches
 *   (t = (i2 / p2) G0 G1 + (i0 / p0) G1 + i1 / p1) -> sums fp32 [B, N, 2]: sums[b, t, 0] the sum and sums[b, t, 1] the sum of the absolute
 *   values of the voxels of patch t, both accumulated in double in a fixed order (the same bits on every run) and stored as fp32. */
int nv_path_points(const float* x, int B, long V, const int* jobs, int J, const float* alphas, int K, float value, const float* base,
                   long base_stride, float* out, void* stream);
int nv_class_score_grads(const float* logits, int J, int C, const int* jobs, const long* cls, int B, int kind, float* dlogits, void* stream);
int nv_path_accumulate(const float* g, const int* jobs, int J, const float* weights, int K, float* acc, int B, long V, void* stream);
int nv_path_finish(const float* acc, const float* x, int B, long V, float value, const float* base, long base_stride, float* attr, void* stream);
int nv_attr_token_sums(const float* attr, int B, const int* size3, const int* patch3, float* sums, void* stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) attribution for the 4D model: the steps that see a
 * series of T volumes per sample.  No call allocates or synchronises; every argument is checked first (NV_ERR_ARG).
 * nv_gradcam_reduce_grouped: nv_gradcam_reduce over V volumes with the min-max normalisation taken over each `group` consecutive volumes
 *   (V a multiple of group; a sample's T timepoints); minmax (optional) [V / group, 2].  group = 1 gives the bits of
 *   nv_gradcam_reduce_per_volume, group = V those of nv_gradcam_reduce.  One launch.
 * nv_series_map_to_volumes: maps [B, T, N] (N = G0 G1 G2, every volume in token order as nv_token_map_to_volume takes it) -> out fp32
 *   [B, S0, S1, S2, T] (NV_SERIES_LAYOUT_SERIES: time innermost, the layout of the model's input) or [B, T, S0, S1, S2]
 *   (NV_SERIES_LAYOUT_FRAMES).  Normalisation, cut and threshold by the rules of nv_token_map_to_volume, taken
 *     NV_SERIES_SCOPE_SERIES  over the T N cells of a sample jointly: one min, one max, one cut (the quantile at position q (T N - 1)) per
 *                             sample, so relative importance across time survives; one workgroup per sample, the keys in LDS;
 *     NV_SERIES_SCOPE_VOLUME  over every volume on its own: the bits of nv_token_map_to_volume on the B T volumes.
 *   The upsampling of layout SERIES writes each output plane (b, x) - S1 S2 T contiguous floats - from one workgroup, with the taps and the
 *   operation order of nv_token_map_to_volume's: out[b, x, y, z, t] of layout SERIES has the bits of out[b, t, x, y, z] of layout FRAMES.
 *   Limits (NV_ERR_ARG beyond): 1 <= T <= 64; N <= 4096; scope SERIES: T N <= 32768 (128 KiB of keys; one workgroup may hold 160 KiB);
 *   layout SERIES: G1 G2 T + 2 S1 + 2 S2 <= 40960 floats of LDS (160 KiB); layout FRAMES: G1 G2 + 2 S1 + 2 S2 <= 16384 and B T <= 65535.
 *   out and workspace 16-byte aligned.  Two launches.  On return the workspace holds [B, T, N] normalised maps, [B, T, N] thresholded maps
 *   and the cuts ([B] for scope SERIES, [B, T] for scope VOLUME), fp32 in this order, which a caller may read.
 * nv_series_leave_one_out: z fp32 [B, T, 2], z_base fp32 [2] -> out fp32 [B (T + 1), T, 2]: row b (T + 1) is z[b], row b (T + 1) + 1 + t is
 *   z[b] with timepoint t replaced by z_base.  A pure select: every bit passes through.
 * nv_temporal_grad_x_input: dx, z fp32 [B, T, 2] -> out fp32 [B, T] = dx[b, t, 0] z[b, t, 0] + dx[b, t, 1] z[b, t, 1], two products and one
 *   sum, each a separately rounded fp32 operation (no FMA). */
#define NV_SERIES_SCOPE_SERIES 0
#define NV_SERIES_SCOPE_VOLUME 1
#define NV_SERIES_LAYOUT_SERIES 0
#define NV_SERIES_LAYOUT_FRAMES 1
long nv_gradcam_grouped_workspace_bytes(int V, int n, int group);
int nv_gradcam_reduce_grouped(const void* act, const float* grad, int V, int n, int d, int group, float* cam, float* minmax, void* workspace,
                              long ws_bytes, void* stream);
long nv_series_map_to_volumes_workspace_bytes(int B, int T, const int* grid3, int scope);
int nv_series_map_to_volumes(const float* maps, int B, int T, const int* grid3, const int* out3, int normalize, int scope, double keep_percent,
                             int layout, float* out, void* workspace, long ws_bytes, void* stream);
int nv_series_leave_one_out(const float* z, const float* z_base, int B, int T, float* out, void* stream);
int nv_temporal_grad_x_input(const float* dx, const float* z, int B, int T, float* out, void* stream);

/* ---- the 4D model's temporal head (src/models/NeuroEncoder.py:60-66: temporal_transformer -> mean over time -> projection_head;
 * :207-217 TemporalTransformer = one nn.TransformerEncoderLayer(d_model 2, nhead 2, batch_first, post-norm, ReLU, dim_feedforward ff,
 * dropout p at its four sites); :219-230 ProjectionHead = nn.Linear(2, 2)) - ONE launch per direction.
 * x [B, T, 2] f32 contiguous (the frozen encoder's logits per timepoint), T <= 64, ff <= 2048; out [B, 2].
 * params / grads: one flat fp32 arena of nv_temporal_head_param_count(ff) = 40 + 5 ff floats in named_parameters() order:
 *   in_proj_weight [6,2] | in_proj_bias [6] | out_proj.weight [2,2] | out_proj.bias [2] | linear1.weight [ff,2] | linear1.bias [ff] |
 *   linear2.weight [2,ff] | linear2.bias [2] | norm1.weight | norm1.bias | norm2.weight | norm2.bias [2 each] |
 *   projection_head.weight [2,2] | projection_head.bias [2].
 * drop_p > 0 (training): counter-based masks from drop_seed; the backward call recomputes the forward from x (nothing else is saved)
 * and must be given the forward's seed and p.  accumulate != 0 adds into grads; dx ([B, T, 2], may be NULL) receives the input gradient. */
long nv_temporal_head_param_count(int ff);
int nv_temporal_head_fwd(const float* x, int B, int T, int ff, const float* params, float eps, unsigned long drop_seed, float drop_p,
                         float* out, void* stream);
int nv_temporal_head_bwd(const float* x, int B, int T, int ff, const float* params, float eps, unsigned long drop_seed, float drop_p,
                         const float* dout, float* grads, int accumulate, float* dx, void* stream);

/* ---- whole-encoder engine: ViT.forward / its backward as ONE call each (vit_3d.py:112-126)
 * Parameters live in one flat fp32 arena (+ a bf16 shadow with identical element offsets) laid out by
 * nv_vit_param_table in the reference's state_dict order; gradients go to an arena of the same layout. */
typedef struct nv_vit_config {
  int image_size, image_patch_size, frames, frame_patch_size;
  int channels, num_classes, dim, depth, heads, dim_head, mlp_dim;
  float ln_eps;
  int pool_mean;   /* 0: pool='cls' (NeuroEncoder.py:194), 1: pool='mean' (vit_3d.py:127) */
  int image_width, patch_width;   /* vit_3d.py:80-81 takes (height, width) pairs: image_size / image_patch_size are the HEIGHTS,
                                     these the widths; 0 = square (the NeuroEncoder path is cubic: NeuroEncoder.py:183-186) */
  int no_proj_dropout;            /* (revision 6) 1: no nn.Dropout behind the output projection - the heads == 1 && dim_head == dim geometry, whose
                                     to_out is nn.Identity() (vit_3d.py:32,43-46); the other three dropout sites of a block are unaffected */
} nv_vit_config;

/* heads == 1 && dim_head == dim: the reference has no output projection (vit_3d.py:32,43-46) but the table still carries every
 * block's to_out weight / bias slot: fill them with the identity / zeros and leave them out of the optimizer (x + I ao + 0 == x + ao
 * exactly, and the data gradient g I == g); neurovit_amd.ViT does that. */
long nv_vit_param_count(const nv_vit_config* cfg);
int nv_vit_param_table(const nv_vit_config* cfg, long* offsets, long* numels, int max_entries);
/* training: 0 = bf16 / fp8 inference layout, 1 = training layout (every layer's activations kept), 2 = fp32 inference layout */
long nv_vit_workspace_bytes(const nv_vit_config* cfg, int B, int training);
/* byte offset of a named activation inside the workspace (-1 if unknown); layer < 0 for global buffers */
long nv_vit_workspace_offset(const nv_vit_config* cfg, int B, int training, const char* name, int layer);
/* shape5 = {B, C, F, H, W} of `video`: must equal {B, cfg.channels, cfg.frames, cfg.image_size, width (cfg.image_width or cfg.image_size)} (the reference
 * fails in einops / the pos_embedding add for any other volume, vit_3d.py:92,118; here a wrong extent would be gathered out of
 * bounds, so it is rejected with NV_ERR_ARG).
 * drop_p / emb_drop_p / drop_seed: nn.Dropout of the blocks (vit_3d.py:21,23,39,45) and of the embedding (:100); both 0
 * in eval mode.  backward must be given the forward's values. */
/* Optional input forms, nv_vit_forward_in / nv_vit_forward_fp8:
 *   vol_sigma   != NULL: `video` holds RAW volumes; [B] (or [B / time_points]) = std + 1e-8 per sample (nv_volume_sigma): the z-score
 *                        is folded into the patch LayerNorm (see nv_patch_ln_fwd); crop = the strides / base pointer of the view;
 *   time_points  > 0   : `video` is a contiguous 4D batch [B / T, H, W, D, T] (shape5 = that shape) and volume b*T + t is timepoint t
 *                        of sample b - no regroup copy (nv_patch_ln_fwd_4d; T % 4 == 0, channels = 1); strides5 is ignored;
 *   rows_form          : which rows of the LAST block's out-projection / LayerNorm / FeedForward are computed - see nv_vit_set_cls_tail.
 *                        A backward must be given the rows_form (and dropout) of its forward. */
/* (revision 8) attention probabilities of the forward, exported behind each layer's attention launch (explainability: the output of
 * the reference's `attend` = nn.Softmax, vit_3d.py:54, which the fused attention kernels never materialise; see nv_attn_probs).
 * maps: HOST array [depth] of device pointers, NULL = that layer is not exported; each receives the nv_attn_probs output of the layer
 * (fusion / rows below) for the forward's B volumes.  Pre-dropout probabilities, whatever the dropout of the forward.  The export only
 * reads the layer's qkv buffer: logits, workspace and every later backward are bit-identical to a forward without it.
 * struct_size = sizeof(nv_vit_attn_export): checked.  The fp8 forwards refuse an export (NV_ERR_ARG). */
typedef struct nv_vit_attn_export {
  int struct_size;
  float** maps;
  int fusion;      /* NV_ATTN_PER_HEAD, NV_ATTN_FUSE_MEAN / _MAX / _MIN */
  int rows;        /* NV_ATTN_ROWS_ALL, NV_ATTN_ROWS_CLS */
} nv_vit_attn_export;
typedef struct nv_vit_input {
  const float* vol_sigma;
  int time_points;
  int rows_form;   /* last block under pool='cls': 0 = process default (nv_vit_set_cls_tail), 1 = every row, 2 = cls rows when eligible */
  const nv_vit_attn_export* attn_export;   /* (revision 8) NULL = no export: exactly the launches of a forward without this field */
} nv_vit_input;
int nv_vit_forward_in(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                      const nv_vit_input* in, const float* params, const void* params16, void* workspace, long ws_bytes,
                      int training, float drop_p, float emb_drop_p, unsigned long drop_seed, float* logits, void* stream);
int nv_vit_forward(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                   const float* params, const void* params16, void* workspace, long ws_bytes, int training, float drop_p, float emb_drop_p,
                   unsigned long drop_seed, float* logits, void* stream);
/* Inference forward with the blocks' LayerNorms folded into the GEMMs around them (nv_gemm_resid_ln / nv_gemm_lnfold above): nv_vit_forward_in(training = 0)
 * without 21 of ViT3D-base's 24 LayerNorm launches (not folded: LN1 of block 0, LN1 of the last block - the Grad-CAM hook tensor - and a last block on its cls
 * rows).  fold16: 16-bit arena (operand format) with the parameter arena's element offsets; fold32: nv_vit_lnfold_floats floats; both filled by
 * nv_vit_lnfold_prepare whenever the parameters have changed.  Falls back to the unfolded launches for shapes outside the LDS-epilogue kernels. */
long nv_vit_lnfold_floats(const nv_vit_config* cfg);
int nv_vit_lnfold_prepare(const nv_vit_config* cfg, const float* params, void* fold16, float* fold32, void* stream);
int nv_vit_forward_lnfold(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5, const nv_vit_input* in,
                          const float* params, const void* params16, const void* fold16, const float* fold32, void* workspace, long ws_bytes,
                          float* logits, void* stream);
/* fp32 inference forward: ViT.forward (vit_3d.py:112-126) as the reference's fp32 validate computes it (Trainer.py:101-118) - every
 * operand fp32 (weights straight from `params`, no shadow arena), contractions on the fp32 MFMA, eval mode (no dropout).
 * Workspace: nv_vit_workspace_bytes(cfg, B, 2).  Input forms as nv_vit_forward_in. */
int nv_vit_forward_f32(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                       const nv_vit_input* in, const float* params, void* workspace, long ws_bytes, float* logits, void* stream);
/* fp8 inference forward (BASELINE.json configs[4] "ViT3D-large ... fp8 MFMA"): all four linears of every block - qkv, the
 * out-projection (its operand written as e4m3 by the attention kernel itself: nv_attn_fwd_o8), FC1, FC2 - on e4m3 operands.
 * act_scales: HOST array [depth][4] (LN1 output, LN2 output, GELU output, attention output - <= 0 keeps that block's out-projection on
 * bf16 operands; calibrated: 448 / (headroom * amax)); params8: byte arena
 * with the element offsets of the parameter arena; colscales: f32 [nv_vit_fp8_scale_count].  Workspace: training = 0 layout. */
long nv_vit_fp8_scale_count(const nv_vit_config* cfg);
int nv_vit_quantize_fp8(const nv_vit_config* cfg, const float* params, const float* act_scales, void* params8, float* colscales, void* stream);
int nv_vit_forward_fp8(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                       const nv_vit_input* in, const float* params, const void* params16, const void* params8, const float* colscales,
                       const float* act_scales, void* workspace, long ws_bytes, float* logits, void* stream);
/* fp8 TRAINING forward: as nv_vit_forward_in(training = 1) - every activation the backward pass reads is written, in bf16 / fp32, where
 * the bf16 forward writes it - with qkv, FC1 and FC2 of every block on e4m3 operands (params8 / colscales / act_scales as for
 * nv_vit_forward_fp8; act_scales[4 l + 3], the out-projection's, is ignored: that linear stays on bf16 operands, as do attention, the
 * patch embedding, the head and a last block in the cls-rows form).  drop_p / emb_drop_p / drop_seed as for nv_vit_forward_in (the masks
 * of the four block sites are those of the bf16 forward: the backward pass recomputes them from the same arguments).
 * Follow it with nv_vit_backward[_stages16] exactly as after nv_vit_forward_in; re-quantise the weights (nv_vit_quantize_fp8) after
 * every optimizer step.  Workspace: the training layout (nv_vit_workspace_bytes(cfg, B, 1)). */
int nv_vit_forward_fp8_train(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                             const nv_vit_input* in, const float* params, const void* params16, const void* params8, const float* colscales,
                             const float* act_scales, void* workspace, long ws_bytes, float drop_p, float emb_drop_p, unsigned long drop_seed,
                             float* logits, void* stream);
int nv_vit_backward(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                    const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads,
                    int accumulate, float drop_p, float emb_drop_p, unsigned long drop_seed, void* stream, void* aux_stream);

/* aux_stream (may be NULL): a second hipStream_t on which the weight-gradient GEMMs run concurrently with the data-gradient
 * chain; the engine forks / joins with pooled events.
 * Backward split into stages (0 = head, 1+k = layer depth-1-k, depth+1 = patch embedding) so the caller can start the
 * data-parallel all-reduce of a stage's gradient range (nv_vit_stage_param_range) while later stages still run.
 * join_aux = 1: the call returns with `stream` ordered after all of its work on both streams.  join_aux = 0 (allowed for
 * ranges that do not contain the last stage): `stream` is NOT made to wait for the auxiliary stream - the range's gradients
 * are complete once BOTH streams have executed what this call enqueued, so the consumer (the all-reduce) must be ordered
 * after both; the next call on the same workspace picks the dependency up where this one left it. */
int nv_vit_backward_stages(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                           const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads,
                           int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p,
                           unsigned long drop_seed, void* stream, void* aux_stream, int join_aux);
/* as nv_vit_backward_stages; grads16 (may be NULL): bf16 arena with the element offsets of `grads` - the weight gradients of the
 * Linear layers (to_qkv, to_out, FC1, FC2 of every block; the patch embedding's when patch_dim % 8 == 0) are ALSO written there,
 * rounded, by the GEMMs that produce them: a data-parallel caller sends them without a cast pass and converts only the small
 * remaining ranges (nv_cast_ranges_bf16). */
int nv_vit_backward_stages16(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                             const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads, void* grads16,
                             int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p,
                             unsigned long drop_seed, void* stream, void* aux_stream, int join_aux, int rows_form);
/* (revision 7) options of nv_vit_backward_ex - the gradient w.r.t. the input volume, and the data-only backward.
 * dvideo (may be NULL): f32 [B, C, F, H, W] with element strides dvideo_strides5 - receives d loss / d video (every element written
 *   exactly once, by the call whose stage range contains the embedding stage, depth + 1; on the auxiliary stream behind the dxp GEMM,
 *   ordered before `stream` by the final join).  Needs the plain input form of the forward (no vol_sigma, no time_points).
 * weight_grads = 0: the data-only backward - none of the work that only produces parameter gradients runs (per-layer weight-gradient
 *   GEMMs, bias / LayerNorm column reductions, the patch embedding's dW, nv_patch_ln_bwd); the data chain, the Grad-CAM hook gradient
 *   (workspace "hookg") and dvideo are bit-identical to a backward with weight_grads = 1.  `grads` and `grads16` must then be NULL:
 *   nothing is written to a gradient arena, and everything runs on `stream` (aux_stream is not used).
 * struct_size = sizeof(nv_vit_backward_opts): checked. */
typedef struct nv_vit_backward_opts {
  int struct_size;
  float* dvideo;
  const long* dvideo_strides5;
  int weight_grads;          /* 1 = parameter gradients as nv_vit_backward_stages16; 0 = data-only */
} nv_vit_backward_opts;
/* nv_vit_backward_stages16 with options (opts = NULL: exactly nv_vit_backward_stages16).  Not for the fused-update path of
 * nv_vit_train_step, nor after a forward of the fused 4D input form (time_points). */
int nv_vit_backward_ex(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                       const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads, void* grads16,
                       int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p,
                       unsigned long drop_seed, void* stream, void* aux_stream, int join_aux, int rows_form, const nv_vit_backward_opts* opts);
/* (added within revision 8 - a new symbol and a new struct, nothing existing changes) nv_vit_backward_ex that also exports the gradient
 * w.r.t. the attention probabilities: for every layer inside the call's stage range whose maps[l] is not NULL, nv_attn_grad (form below)
 * is queued on `stream` right behind that layer's nv_attn_bwd, while the workspace still holds its dAO and qkv.  maps: HOST array [depth]
 * of device pointers, NULL = that layer is not exported; each receives [B, heads, n, n] (per head) or [B, n, n] (relevance) fp32.
 * Works in the full and in the data-only backward (opts->weight_grads = 0), whole or staged; every other output is bit-identical to a
 * backward without it, and attn_grad = NULL is exactly nv_vit_backward_ex.  Under pool = 'cls' with the last block on its cls rows the
 * last layer's map is zero outside row 0 (only the cls row reaches the head).
 * Refused (NV_ERR_ARG): drop_p > 0 (the attention-dropout mask is not replayed into dP), a wrong struct_size, a NULL maps array. */
typedef struct nv_vit_attn_grad_export {
  int struct_size;           /* sizeof(nv_vit_attn_grad_export) */
  float** maps;
  int form;                  /* NV_ATTN_GRAD_PER_HEAD, NV_ATTN_GRAD_RELEVANCE */
} nv_vit_attn_grad_export;
int nv_vit_backward_attn(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                         const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads, void* grads16,
                         int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p,
                         unsigned long drop_seed, void* stream, void* aux_stream, int join_aux, int rows_form, const nv_vit_backward_opts* opts,
                         const nv_vit_attn_grad_export* attn_grad);
/* (added within revision 8 - a new symbol, nothing existing changes) the backward from a gradient on the FINAL TOKENS instead of the
 * logits: nv_vit_backward_ex's arguments with dtokens fp32 [B n, dim] dense (16-byte aligned) in the place of dlogits - the gradient
 * w.r.t. the last block's output, cls rows included.  Any token-level objective (masked reconstruction, distillation on tokens,
 * contrastive patch losses) differentiates the encoder through it.  Stage 0 of the range is a seeding launch (nv_token_grad_seed) in
 * the head's place: it leaves what nv_head_bwd leaves for stage 1 - the running residual gradient g = dtokens, the last layer's 16-bit
 * gradient cvt(dtokens * mask) under the dropout mask of site 4 (depth - 1) + 3, and the last layer's FC2 bias gradient = the column sums
 * of dtokens * mask (per-workgroup partials, then nv_reduce_multi: a fixed order) - and stages 1 .. depth + 1 are those of nv_vit_backward_ex.
 * The head takes no part: its gradient range (nv_vit_stage_param_range of stage 0) is written as zeros with accumulate = 0 and left
 * alone with accumulate = 1 (the full form; the data-only form writes no arena).  opts and grads16 behave as in nv_vit_backward_ex.
 * The forward must have run its last block on EVERY row (nv_vit_input.rows_form = 1) and the same value must arrive here: refused
 * (NV_ERR_ARG) when these arguments select the cls-rows form, and for a NULL or misaligned dtokens.  Not after a forward of the fused 4D
 * input form (as nv_vit_backward_ex). */
int nv_vit_backward_tokens(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                           const void* params16, void* workspace, long ws_bytes, const float* dtokens, float* grads, void* grads16,
                           int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p,
                           unsigned long drop_seed, void* stream, void* aux_stream, int join_aux, int rows_form, const nv_vit_backward_opts* opts);
int nv_vit_stage_param_range(const nv_vit_config* cfg, int stage, long* begin, long* end);
/* pool='cls': the last block's out-projection / LayerNorm / FeedForward, forward and backward, on the B cls rows only (whenever the
 * block dropout is off; training additionally B <= 4).  Logits and every gradient are unchanged (the other rows never reach the
 * head and receive exact zeros in the backward pass), but rows 1..n-1 of the last block's x1 / xn2 / u / h / x2 workspace buffers
 * are not produced.  The form is chosen PER CALL by rows_form (nv_vit_input / nv_vit_backward_stages16); this sets the process
 * default used by rows_form = 0 and by the entry points without that argument: 1 (initial) = cls rows, 0 = every row. */
int nv_vit_set_cls_tail(int on);
int nv_vit_set_head_step(int on);   /* A/B aid: 0 = nv_vit_train_step runs the head as nv_head_fwd + nv_ce_loss + nv_head_bwd (same bits), 1 (default) = nv_head_step */

/* ---- the reference's whole train step (src/Trainer.py:65-79) as ONE call: ViT forward (training layout) -> nn.CrossEntropyLoss
 * (mean) -> backward of every stage -> torch.optim.AdamW update of the whole arena (+ bf16 shadow refresh).  ~225 kernel launches
 * enqueued from native code with no interpreter in between; nothing synchronises, `loss` and `logits` stay on the device.
 * hp: see the struct (struct_size = sizeof(nv_train_hparams): checked, NV_ERR_ARG on mismatch).  labels: int64 [B].
 * logits / dlogits: f32 [B, num_classes] (dlogits is scratch the backward reads); loss: f32 [1].
 * accumulate = 1: gradients are added to `grads` (micro-steps 2.. of an accumulation window); update = 0: no optimizer update
 * (every micro-step but the last).  The arguments a separate backward would need (rows_form of `in`, dropout) are the forward's
 * by construction. */
/* ---- data-parallel train step from native code (no counterpart in the reference, which is single-device: main.py:41-46).
 * RCCL is bound at run time (dlopen; nv_comm_load(path) names the copy to use - the one torch's "nccl" backend has loaded - or NULL for
 * the default search).  Communicator: rank 0 calls nv_comm_unique_id (128 bytes), every rank receives those bytes over a channel of its
 * own (one torch.distributed broadcast) and calls nv_comm_init.  nv_comm_all_reduce: in-place SUM on `stream`; dtype 0 = f32, 1 = the
 * 16-bit operand format.
 * nv_dp_plan (nv_train_hparams.dp): the backward pass of nv_vit_train_step runs as n_buckets groups of stages; as soon as a group has
 * been enqueued, comm_stream waits for it and all-reduces the group's (contiguous) gradient range while the main stream continues -
 * fp32 in `grads` itself, or, with grads16 != NULL, as 16-bit messages in that arena (the Linear weight gradients are written there by
 * their GEMMs, the small ranges are converted on comm_stream).  update_per_bucket = 1 queues AdamW of that range (grad * grad_scale /
 * world) behind its all-reduce on comm_stream; 2 = on aux_stream, one bucket late (in front of the next bucket's weight-gradient work,
 * once the all-reduce has finished: the update then never runs beside the weight-gradient GEMMs; the last bucket's on `stream`);
 * 0 = one update over the arena when every bucket is in.  With grads16 the update reads
 * the reduced messages and `grads` keeps the LOCAL gradients.  Micro-steps with update = 0 run no collective. */
typedef struct nv_dp_plan {
  int struct_size;
  int world;               /* ranks: the update scales the summed gradients by 1 / world */
  void* comm;              /* nv_comm_init */
  void* comm_stream;       /* hipStream_t of the collectives; must not share a hardware queue with `stream` / `aux_stream` for overlap */
  int n_buckets;           /* 1 .. depth + 2 */
  int update_per_bucket;
  void* grads16;           /* NULL = fp32 messages */
} nv_dp_plan;
int nv_comm_load(const char* path);
int nv_comm_unique_id(void* id128);
int nv_comm_init(const void* id128, int world, int rank, void** comm);
int nv_comm_destroy(void* comm);
int nv_comm_all_reduce(void* comm, void* buf, long count, int dtype, void* stream);

typedef struct nv_train_hparams {
  int struct_size;
  int step;                 /* AdamW step count (>= 1) of this update: bias corrections (ignored when update = 0) */
  double lr, beta1, beta2, eps, weight_decay;
  float grad_scale;         /* the update reads grad * grad_scale */
  int accumulate, update;
  int fuse_update;          /* (revision 5) with update = 1, accumulate = 0: where the Linear weights of the transformer layers (96 % of the
                             * parameters) are updated.  0 = with everything else, one nv_adamw_step behind the backward pass.
                             * 3 = per layer, by an AdamW launch on the auxiliary stream behind that layer's weight-gradient GEMMs, while
                             * the main stream is already in the next layer (gradients stay in `grads`).  1 = by the weight-gradient GEMMs
                             * themselves (nv_gemm_bf16_grouped_adamw; the gradients of those weights are then NOT left in `grads`),
                             * 2 = the same and they are.  In 1 .. 3 the rest of the arena is updated by one nv_adamw_ranges launch.
                             * Parameters, optimizer state and losses are bit-identical in all four */
  float loss_scale;         /* (revision 6) static loss scale: d(loss)/d(logits) is multiplied by it and the update divides it out again
                             * (0 or 1 = none) - what keeps the 16-bit gradient tensors of NV_OPERAND_FP16 away from the subnormals; a power
                             * of two changes no bit of a finite result.  No overflow check: use loss_scale_state for GradScaler semantics */
  const struct nv_dp_plan* dp;   /* (revision 6) data-parallel step: NULL, or the plan below */
  float* loss_scale_state;  /* (revision 6) device block of nv_loss_scale_init or NULL: dynamic loss scale (torch.amp.GradScaler, Trainer.py:29,
                             * 74-76) - the step is scaled by its current value, every gradient is checked for inf / NaN after the backward
                             * pass, and the update is applied or skipped on the device (requires fuse_update = 0; with accumulate / update
                             * = 0 micro-steps only the scaling happens) */
} nv_train_hparams;
int nv_vit_train_step(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5, const nv_vit_input* in,
                      float* params, void* params16, float* grads, float* adam_m, float* adam_v, void* workspace, long ws_bytes,
                      const long* labels, float* logits, float* loss, float* dlogits, const nv_train_hparams* hp,
                      float drop_p, float emb_drop_p, unsigned long drop_seed, void* stream, void* aux_stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) training augmentation on the device: a per-sample
 * random crop (monai's RandSpatialCrop with a fixed size: the reference's DATASET_TRANSFORMS), integer translation, axis flips and an affine
 * intensity change, for 3D volumes and 4D series.  No call allocates, synchronises or reads anything back, and the host draws no random
 * number; every argument is checked first (NV_ERR_ARG: a NULL pointer, sizes that are not positive, a roi larger than the input, a wrong
 * struct_size, a probability outside [0, 1], lo > hi, a negative max_shift or rank).
 * nv_augment_params: writes params int32 [B, 8] (DEVICE), row b = {ox, oy, oz, flips (bit 0 / 1 / 2 = x / y / z), bits of the fp32 scale,
 *   bits of the fp32 shift, 0, 0}.  The draw rule, with nv_hash64 the 64-bit hash of the dropout masks
 *   (x = (c + 0x9E3779B97F4A7C15) * 0xBF58476D1CE4E5B9 ^ seed; x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27;
 *   x *= 0x94D049BB133111EB; x ^= x >> 31, all mod 2^64, for nv_hash64(seed, c)):
 *     seed_r = nv_hash64(seed, rank);  draw d of sample b at step s:  h = nv_hash64(seed_r, ((s 2^32 + b) 16 + d) mod 2^64)
 *     an integer on [0, n):        ((h >> 32) n) >> 32        (no rejection; the bias is below 2^-32 n)
 *     crop offset, axis a (d = a):             uniform on [0, in_size[a] - roi[a]]
 *     translation, axis a (d = 3 + a):         uniform on [-max_shift[a], max_shift[a]] (an integer on [0, 2 m + 1) minus m), ADDED to the
 *                                              crop offset: the window may leave the volume
 *     flip, axis a (d = 6 + a):                (h >> 48) < (unsigned)(flip_prob[a] * 65536), the product in double: never for 0, always for 1
 *     scale (d = 9), shift (d = 10):           u = (h >> 40) 2^-24 (exact in fp32); lo + ((hi - lo) u), the difference, the product and the
 *                                              sum each rounded to fp32 on its own (no FMA)
 * nv_augment_apply: src fp32 [B, X, Y, Z, T] with the element strides strides5 (HOST array of 5; any strides, T = 1 for volumes), in3 =
 *   {X, Y, Z} and roi3 = {Sx, Sy, Sz} HOST arrays, params int32 [B, 8] (DEVICE, rows as above; offsets may be anything)
 *   -> out fp32 [B, Sx, Sy, Sz, T] dense, 16-byte aligned.  With s_a = o_a + (flip_a ? S_a - 1 - i_a : i_a) per axis:
 *     out[b, i, j, k, t] = (src[b, sx, sy, sz, t] * scale) + shift   inside the volume (two roundings, no FMA)
 *                        = fill, verbatim                            outside it
 *   The T timepoints of a sample share its row.  A sample whose scale is exactly 1.0f and whose shift is exactly 0.0f is a bit copy (NaN
 *   payloads, -0.0).  Every output element is written exactly once, nothing else is written; one launch whose grid follows the output
 *   rows (B Sx planes), 16-byte stores whatever the alignment of the rows.  Limits (NV_ERR_ARG beyond): B Sx < 2^31, Sy Sz T <= 65535 * 4096. */
typedef struct {
  int struct_size;            /* sizeof(nv_augment_config): checked */
  int in_size[3];             /* X, Y, Z of the input volume */
  int roi[3];                 /* Sx, Sy, Sz of the window */
  int max_shift[3];
  double flip_prob[3];
  float scale_lo, scale_hi, shift_lo, shift_hi;
} nv_augment_config;
int nv_augment_params(const nv_augment_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* params, void* stream);
int nv_augment_apply(const float* src, const long* strides5, int B, const int* in3, int T, const int* params, const int* roi3, float fill,
                     float* out, void* stream);

/* (added within revision 8 - new symbols and new structs only, nothing existing changes) the other half of a ViT training recipe:
 * a soft-target cross-entropy (label smoothing, class weights, a Mixup / CutMix target) and the mixing pass itself.
 *
 * ---- the loss.  With y_a = labels[b], y_b = labels[partner_b] and lam_b the row's label lambda (fp32), both read from row b of `mix`
 * (y_b = y_a, lam_b = 1 without one):
 *     q_b  = lam_b onehot(y_a) + (1 - lam_b) onehot(y_b)         q'_b = (1 - eps) q_b + eps / C         p_b = softmax(z_b)
 *     loss = ( sum_b sum_c w_c q'_bc (-log p_bc) ) / D
 *     D    = sum_b sum_c w_c q_bc                                (UNsmoothed: sum_b w[y_b] without a mix, B without weights)
 *     dloss/dz_bc = ( p_bc S_b - w_c q'_bc ) / D,  S_b = sum_c w_c q'_bc      (times grad_scale, times state[0] with a loss-scale state)
 *   Without a mix this is F.cross_entropy(z, y, weight=w, label_smoothing=eps) (torch's index-target form, which divides by sum w[y]);
 *   without weights and with a mix it is F.cross_entropy(z, q, label_smoothing=eps) (torch's probability-target form, which divides by
 *   B).  With both, torch's two forms disagree about the denominator; THE RULE ABOVE IS THIS PROJECT'S: the unsmoothed weight of the
 *   mixed target.  D is formed in double in a fixed order; D == 0 gives a NaN loss.  A label - the row's own or its partner's - outside
 *   [0, C), or a partner outside [0, B), gives a NaN loss; nothing is read through an unchecked index.
 *   opts == NULL, or every option off (label_smoothing 0, both pointers NULL), IS nv_ce_loss_scaled / nv_head_step_scaled /
 *   nv_vit_train_step: the call is handed to them (same launches, same bits).  nv_ce_loss_soft and nv_head_step_soft share one row
 *   body and give the same bits.  Refused (NV_ERR_ARG) before any launch: a wrong struct_size, label_smoothing outside [0, 1).
 *   nv_vit_train_step_ex takes every nv_train_hparams form of nv_vit_train_step, on both head routes. */
#define NV_MIX_COLS 12
typedef struct nv_loss_opts {
  int struct_size;              /* sizeof(nv_loss_opts): checked */
  float label_smoothing;        /* eps in [0, 1) */
  const float* class_weight;    /* device f32 [C] or NULL (= all ones) */
  const int* mix;               /* device int32 [B, NV_MIX_COLS] rows of nv_mix_params or NULL: partner (column 0) and label lambda (column 3) are read */
} nv_loss_opts;
int nv_ce_loss_soft(const float* logits, const long* target, int B, int C, float grad_scale, const float* scale_state, const nv_loss_opts* opts,
                    float* loss, float* dlogits, void* stream);
int nv_head_step_soft(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps, const float* W,
                      const float* bias, int C, const long* labels, float grad_scale, const float* scale_state, const nv_loss_opts* opts,
                      float* xh, float* stats, float* logits, float* loss, float* dlogits, int n, float* g, long ldg, void* g16, long ldg16,
                      float* dgamma, float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                      unsigned long drop_seed, float drop_p, void* stream);
int nv_vit_train_step_ex(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5, const nv_vit_input* in,
                         float* params, void* params16, float* grads, float* adam_m, float* adam_v, void* workspace, long ws_bytes,
                         const long* labels, float* logits, float* loss, float* dlogits, const nv_train_hparams* hp, const nv_loss_opts* lo,
                         float drop_p, float emb_drop_p, unsigned long drop_seed, void* stream, void* aux_stream);

/* ---- nv_mix_params: writes mix int32 [B, NV_MIX_COLS] (DEVICE), row b = {partner, mode (0 none, 1 mixup, 2 cutmix), bits of the pixel
 *   lambda, bits of the label lambda, tries, x0, x1, y0, y1, z0, z1, 0}.  One thread per sample, nothing is read back, the host draws no
 *   random number.  The draws live in a domain of their own (no augmentation draw is reused), with nv_hash64 as for nv_augment_params:
 *     seed_m = nv_hash64(nv_hash64(seed, rank), 0x4D4958);  draw d of sample b at step s:  h_d = nv_hash64(seed_m, ((s 2^32 + b) 256 + d) mod 2^64)
 *     partner = B - 1 - b (timm's flip(0)); a sample that is its own partner (the middle of an odd batch, B = 1) has mode 0.
 *     applied (d = 0):  (h >> 48) < (unsigned)(prob * 65536), the product in double; otherwise mode 0.
 *     mode (d = 1):     with both alphas set, cutmix iff (h >> 48) < (unsigned)(switch_prob * 65536), else mixup; with one alpha, its mode;
 *                       with none, mode 0.  alpha = 0 means "not set"; a set alpha lies in [0.05, 1].
 *     lambda ~ Beta(alpha, alpha) by Joehnk's rule in DOUBLE: try t < 64 uses u from d = 16 + 2 t and v from d = 17 + 2 t,
 *                       u = ((h >> 12) + 0.5) 2^-52 (exact, never 0); x = pow(u, 1 / alpha), y = pow(v, 1 / alpha); the first t with
 *                       x + y <= 1 is accepted (after 64 rejections the last pair is used: probability <= 2^-64);
 *                       lambda = (float)(x / (x + y)), tries = t + 1.  This is the pixel lambda.
 *     mixup:            label lambda = pixel lambda, the box columns are 0.
 *     cutmix box, in FP32, in output-window coordinates, shared by the T timepoints: r = sqrt(1.0f - lambda) (correctly rounded);
 *                       per axis a: e_a = (int)((float)S_a * r), centre c_a = ((h >> 32) S_a) >> 32 with d = 2 + a,
 *                       lo_a = max(c_a - e_a / 2, 0), hi_a = min(c_a + e_a / 2, S_a) (integer division);
 *                       label lambda = (float)(1 - cells / (Sx Sy Sz)) with cells = prod (hi_a - lo_a), in double, rounded once (an empty box: 1).
 *     mode 0 rows:      {partner, 0, bits of 1.0f, bits of 1.0f, 0, 0 ...}.
 *   Refused (NV_ERR_ARG): NULL pointers, B < 1, a negative rank, a wrong struct_size, a roi that is not positive, a set alpha outside
 *   [0.05, 1] (above 1 Joehnk's acceptance rate falls below one half, below 0.05 u^(1/alpha) underflows), prob / switch_prob outside [0, 1].
 * ---- nv_augment_mix: nv_augment_apply and the mix in ONE streaming launch.  src, strides5, in3, T, roi3, fill, out as for
 *   nv_augment_apply; aug = the rows [B, 8] of nv_augment_params, or NULL for identity rows (offset 0, no flip, scale 1, shift 0); mix =
 *   the rows above (DEVICE).  Write A_b(i, j, k, t) for the cell nv_augment_apply writes for sample b (own crop, flip, fill, (x scale) +
 *   shift in two roundings) and A_p for the same cell of the PARTNER under the partner's own row.  Then out[b, i, j, k, t] is
 *     mode 0, pixel lambda == 1.0f, or a partner outside [0, B):   A_b, a bit copy; the partner is not read
 *     mixup:    (lambda A_b) + (mu A_p), mu = 1.0f - lambda rounded once per sample; two products and one sum, each rounded (no FMA)
 *     cutmix:   A_p verbatim for x0 <= i < x1, y0 <= j < y1, z0 <= k < z1 and A_b verbatim elsewhere (bit moves: NaN payloads, -0.0)
 *   Every output element is written exactly once, nothing else is written; layout, limits and refusals as nv_augment_apply. */
typedef struct nv_mix_config {
  int struct_size;            /* sizeof(nv_mix_config): checked */
  int roi[3];                 /* Sx, Sy, Sz of the output window: the cutmix box lives in it */
  double mixup_alpha;         /* 0 = off, else [0.05, 1] */
  double cutmix_alpha;        /* 0 = off, else [0.05, 1] */
  double prob, switch_prob;
} nv_mix_config;
int nv_mix_params(const nv_mix_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* mix, void* stream);
int nv_augment_mix(const float* src, const long* strides5, int B, const int* in3, int T, const int* aug, const int* mix, const int* roi3, float fill,
                   float* out, void* stream);

/* (added within revision 8 - new symbols and one new struct only, nothing existing changes) random affine augmentation on the device:
 * per sample a rotation about the centre of the window, a zoom and a sub-voxel translation on top of the crop, the flips and the
 * intensity change of nv_augment_*, by ONE streaming gather pass with trilinear interpolation, for 3D volumes and 4D series (monai's
 * RandAffine / RandRotate / RandZoom, the neighbours of the reference's RandSpatialCrop).  No call allocates, synchronises or reads
 * anything back, and the host draws no random number; every argument is checked first.
 *
 * ---- nv_affine_params: writes table int32 [B, 16] (DEVICE).  Row b: columns 0 .. 11 the fp32 bit patterns of the 3 x 4 map, as
 *   M_a0, M_a1, M_a2, m_a3 for axis a = x, y, z; column 12 / 13 the bits of the fp32 intensity scale / shift; column 14 flags (bit 0 / 1 / 2 =
 *   flip of x / y / z, bit 3 = affine applied); column 15 zero.  The map takes output cell (i, j, k) of the window to a source coordinate
 *   in voxel units of the input volume: s_a = M_a0 i + M_a1 j + M_a2 k + m_a3.
 *   The draws live in a domain of their own (no draw of nv_augment_params or nv_mix_params is reused), with nv_hash64 as above:
 *     seed_f = nv_hash64(nv_hash64(seed, rank), 0x414646);  draw d of sample b at step s:  h = nv_hash64(seed_f, ((s 2^32 + b) 32 + d) mod 2^64)
 *     a real u = (h >> 11) 2^-53, exact in double
 *     d = 0 .. 2     crop offset o_a: an integer on [0, in_size[a] - roi[a]], ((h >> 32) n) >> 32 as nv_augment_params
 *     d = 3 .. 5     flip of axis a: (h >> 48) < (unsigned)(flip_prob[a] * 65536)
 *     d = 6          applied iff (h >> 48) < (unsigned)(prob * 65536)
 *     d = 7 .. 9     theta_a = (2 u - 1) rotate_deg[a] (pi / 180)
 *     d = 10 .. 12   z_a = zoom_lo + (zoom_hi - zoom_lo) u; with `isotropic`, d = 10 serves all three axes
 *     d = 13 .. 15   t_a = (2 u - 1) translate[a], in voxels
 *     d = 16, 17     scale and shift: lo + ((hi - lo) u) in fp32 with u = (h >> 40) 2^-24, as nv_augment_params
 *   A sample that is not applied has theta = 0, z = 1, t = 0 (its rotation is the identity matrix itself); its crop, flips and
 *   intensity still hold.  Then, in DOUBLE, every product and sum rounded on its own, sums from the left:
 *     R = Rz(theta_z) (Ry(theta_y) Rx(theta_x)),  M_ab = R_ab (f_b / z_b) with f_b = -1 for a flipped axis and +1 otherwise
 *     c_a = (roi[a] - 1) / 2,  m_a3 = ((o_a + t_a) + c_a) - ((M_a0 c_x + M_a1 c_y) + M_a2 c_z)
 *   and each of the twelve numbers is rounded to fp32 once (a zero is stored as +0.0).  Zoom z > 1 magnifies the content: the source
 *   step is 1 / z.  The window turns about its own centre, which the crop offset and the translation place in the volume.
 *   Refused (NV_ERR_ARG): NULL pointers, B < 1, a negative rank, a wrong struct_size, a roi that is not positive or larger than the input,
 *   an input beyond 2^24 cells along an axis, |rotate_deg| > 180, zoom not 0 < lo <= hi <= 16, a negative or non-finite translate,
 *   probabilities outside [0, 1], intensity ranges with lo > hi or not finite.
 *
 * ---- nv_affine_apply: src, strides5, B, in3, T, roi3, fill, out as for nv_augment_apply; table int32 [B, 16] (DEVICE) rows as above -
 *   they may also be written by hand and hold anything (NaN, infinities, 1e30).  THE ARITHMETIC IS PART OF THE ABI: all fp32, every
 *   operation rounded on its own, nothing contracted.  For output cell (i, j, k, t) of sample b:
 *     coordinate   s_a = ((M_a0 i + M_a1 j) + M_a2 k) + m_a3, from the indices of every cell (never advanced incrementally)
 *     fraction     f_a = floorf(s_a), w_a = s_a - f_a  (in [0, 1]; 1 is possible just below an integer)
 *     corners      (f_x + dx, f_y + dy, f_z + dz), dx, dy, dz in {0, 1}: inside the volume the source value, outside it `fill`.  The range
 *                  test is made on the FLOAT: a coordinate that is NaN, infinite or not in [-1, N_a) puts the corners it addresses
 *                  outside; no index is formed from an unchecked value
 *     lerp         lerp(a, b, w) = a + ((b - a) w); for w == 0 it is `a` VERBATIM: the upper corners along that axis are not used (a NaN or
 *                  an infinity there does not reach the cell; a fetch of them is from an index clamped into the volume and is discarded)
 *     order        along z first, then y, then x
 *     all outside  a cell whose every USED corner lies outside the volume is `fill`, verbatim
 *     intensity    every other cell becomes (v scale) + shift (two roundings), skipped for scale == 1.0f && shift == 0.0f
 *   Hence a table with an integer map (no rotation, zoom 1, no translation) writes, bit for bit, what nv_augment_apply writes for the
 *   row {m_x3, m_y3, m_z3 (minus S_a - 1 on a flipped axis), flips, scale, shift} - NaN payloads and -0.0 included - and an exact quarter
 *   turn is an exact permutation.  The T timepoints of a sample share its row; each corner of a series cell is T floats.
 *   Every output element is written exactly once, nothing else is written; one launch whose grid follows the output rows.  Limits and
 *   refusals as nv_augment_apply; also refused: an input beyond 2^24 cells along an axis (indices are exact in fp32), an `out` that
 *   overlaps the span of memory `src` and its strides reach (a gather must not overwrite its own source). */
typedef struct nv_affine_config {
  int struct_size;            /* sizeof(nv_affine_config): checked */
  int in_size[3];             /* X, Y, Z of the input volume */
  int roi[3];                 /* Sx, Sy, Sz of the window */
  double rotate_deg[3];       /* theta_a uniform on [-rotate_deg[a], rotate_deg[a]] degrees, about axis a */
  double zoom_lo, zoom_hi;    /* 0 < lo <= hi <= 16 */
  int isotropic;              /* one zoom draw for the three axes */
  double translate[3];        /* t_a uniform on [-translate[a], translate[a]] voxels */
  double prob;                /* probability that rotation / zoom / translation apply to a sample */
  double flip_prob[3];
  float scale_lo, scale_hi, shift_lo, shift_hi;
} nv_affine_config;
int nv_affine_params(const nv_affine_config* cfg, unsigned long seed, unsigned long step, int rank, int B, int* table, void* stream);
int nv_affine_apply(const float* src, const long* strides5, int B, const int* in3, int T, const int* table, const int* roi3, float fill,
                    float* out, void* stream);

/* (added within revision 8 - new symbols only; a caller finds out by symbol lookup) masked-volume pretraining (SimMIM / MAE on volumes): the
 * device steps around the encoder's forward and its token-level backward (nv_vit_backward_tokens).  No call allocates, synchronises or reads
 * anything back, and the host draws no random number; every argument is checked first (NV_ERR_ARG).
 * nv_mim_labels: writes labels int32 [B, N] (DEVICE), N = G0 G1 G2 <= 4096 patches of the grid grid3 = {G0, G1, G2} (HOST array; patch
 *   indices by nv_mask_patches' token rule, t = g2 G0 G1 + g0 G1 + g1).  Per sample a permutation of 0 .. N - 1 in which label < m means
 *   masked: nv_mask_patches with the job (b, 0, m) writes the masked batch.  A mask unit is a cube of u^3 patches (`unit` = u divides
 *   G0, G1 and G2; U_a = G_a / u, U = U0 U1 U2 >= 2 units, indexed q = (g2 / u) U0 U1 + (g0 / u) U1 + g1 / u).  The draw rule, with
 *   nv_hash64 as for nv_augment_params, in a domain of its own (no augmentation draw is reused):
 *     seed_p = nv_hash64(nv_hash64(seed, rank), 0x4D494D);  h_q = nv_hash64(seed_p, ((s 2^32 + b) 4096 + q) mod 2^64)  for unit q of sample b at step s
 *     key_q = (h_q >> 40) 2^-24 (exact in fp32);  rank_q = #{ j : key_j > key_q or (key_j == key_q and j < q) }   (nv_token_ranks' rule)
 *     labels[b, t] = rank_q(t) u^3 + ((g2 mod u) u + g0 mod u) u + g1 mod u
 *   so the first m_u = clamp(floor(ratio U + 0.5), 1, U - 1) units in rank order are masked, as whole cubes, and the masked-patch count
 *   m = m_u u^3 is exact and known on the host: nv_mim_masked_count (ratio in (0, 1); NV_ERR_ARG = -1 otherwise).  A step can be replayed
 *   from (seed, rank, step); ranks and steps draw different masks.  One workgroup per sample, keys ranked in LDS.
 * nv_recon_loss: pred fp32 [B n, ldp] (n = N + 1 token rows per sample, row 0 the cls row; ldp >= P8 = 8 ceil(P / 8), P = p0 p1 p2, a
 *   multiple of 4, 16-byte aligned), the ORIGINAL dense volume x fp32 [B, S0, S1, S2] (size3 / patch3 HOST arrays as for nv_mask_patches,
 *   P <= 4096), labels int32 [B, N] and m as above, kind NV_RECON_L1 / NV_RECON_L2, norm_pix 0 / 1, loss_scale > 0.
 *   For every masked row (labels[b, t] < m, row b n + 1 + t) the target is patch t in the engine's patchify order - element
 *   (a0 p1 + a1) p2 + a2 is voxel (g0 p0 + a0, g1 p1 + a1, g2 p2 + a2), the '(p1 p2 pf c)' order of vit_3d.py:92 with c = 1 - and with
 *   norm_pix it is standardised by the patch mean and the UNBIASED variance, (v - mean) / sqrt(var + 1e-6) (MAE's rule), the statistics
 *   and everything behind them in double.  With diff = pred - target:
 *     loss  = sum |diff| / (B m P)  or  sum diff^2 / (B m P)
 *     dpred = loss_scale sign(diff) / (B m P)  or  loss_scale 2 diff / (B m P), rounded ONCE to the operand format (nv_operand_format)
 *   dpred [B n, ldd] (16-bit, ldd >= P8 a multiple of 8, 16-byte aligned): every other cell - cls rows, rows that are not masked, columns
 *   P .. ldd - 1 - is written as zero, every cell exactly once; pred is not read on those rows.  partials double [B n]: the rows' loss
 *   terms (0 for rows that are not masked); a second launch of one workgroup sums them in index order into loss fp32 [1] (the loss is
 *   NOT multiplied by loss_scale).  One workgroup per row; the patch is read once (16-byte loads when x is 16-byte aligned and S2 and p2
 *   are multiples of 4, dwords otherwise) and kept in LDS between the statistics and the loss pass.  No atomics: the same bits on every run.
 * nv_token_grad_seed: dtokens fp32 [M, d] dense -> g fp32 [M, d] = dtokens, g16 [M, d] (operand format) = cvt(dtokens * mask) with the
 *   dropout mask (drop_seed, drop_p) of the dense [M, d] tensor (element row d + col, as nv_ln_bwd applies it; drop_p = 0: none), and
 *   partials fp32 [nv_token_grad_seed_rows(M), d] (may be NULL) = per-workgroup column sums of dtokens * mask, to be summed by
 *   nv_reduce_multi.  The launch in front of the encoder's backward when the loss sits on its tokens (nv_vit_backward_tokens). */
#define NV_RECON_L1 0
#define NV_RECON_L2 1
int nv_mim_masked_count(const int* grid3, int unit, double ratio);
int nv_mim_labels(unsigned long seed, unsigned long step, int rank, int B, const int* grid3, int unit, int* labels, void* stream);
int nv_recon_loss(const float* pred, long ldp, const float* x, int B, const int* size3, const int* patch3, const int* labels, int m, int kind,
                  int norm_pix, float loss_scale, void* dpred, long ldd, double* partials, float* loss, void* stream);
long nv_token_grad_seed_workspace_bytes(int M, int d);
int nv_token_grad_seed_rows(int M);
int nv_token_grad_seed(const float* dtokens, int M, int d, float* g, void* g16, float* partials, long partial_bytes, unsigned long drop_seed,
                       float drop_p, void* stream);

/* (added within revision 8 - new symbols and one new struct only, nothing existing changes) stochastic depth (drop path; timm's DropPath, the
 * drop_path_rate of the DeiT / BEiT / MAE recipes) in the training forward, the backward and the one-call train step.  For block l (0-based),
 * branch c (0 attention, 1 FeedForward) and sample b:   x <- x + f[l, c, b] * Dropout(branch(LN(x)))   with f a DEVICE table of fp32
 * factors [depth][2][B], each 0 or 1 / (1 - q_l).  A site has an element-dropout factor e (0 or 1 / (1 - p), the rule of nv_gemm_bf16) and
 * the sample's path factor f: every kernel forms k = e * f FIRST, as one fp32 product, and uses k exactly where it uses e without a table -
 * so f == 1.0f gives the bits of the call without a table, f == 0 gives resid + 0, and forward and backward see the same k.  In the
 * backward the 16-bit gradient handed to a branch and the column sums that become its bias gradient are formed from g * k; the fp32
 * running residual gradient g is not scaled.  Dropped branches are still computed (skipping them would need a host read of the draw).
 * nv_drop_path_draw: writes factors[depth][2][B] on the device; nothing is read back, the host draws nothing.
 *   q_l: NV_DROP_PATH_LINEAR  rate * l / (depth - 1) in double (timm's linspace(0, rate, depth); 0 when depth == 1), NV_DROP_PATH_CONSTANT  rate
 *   seed_p = nv_hash64(seed, 0x50415448);  h = nv_hash64(seed_p, ((uint64)(2 l + c) << 32) + b)          (a hash domain of its own)
 *   kept iff (h >> 48) >= (unsigned)(q_l * 65536.0) (the product in double, truncated);  f = 1.0f / (1.0f - (float)q_l) when kept, else 0;
 *   a site whose threshold is 0 writes 1.0f without hashing.  NV_ERR_ARG: rate outside [0, 1), an unknown schedule, B or depth <= 0, factors NULL.
 * Kernel level: the argument lists of nv_gemm_bf16 / nv_skinny_nt / nv_ln_bwd / nv_head_bwd / nv_head_step_soft plus (path, path_rows): path
 *   = the [samples] factors of ONE site, path_rows = token rows per sample.  Row r of a launch is dense row r * (ld / width) of the tensor it
 *   writes (a view of) - ldo / N for nv_skinny_nt_path, ldg / d for nv_ln_bwd_path, 1 for the GEMM - and its sample is that dense row /
 *   path_rows (samples * path_rows < 2^31).  nv_gemm_bf16_path: layout 0, epilogue 4 only; nv_skinny_nt_path: epilogue 0 only; the head forms:
 *   path_rows == n.  nv_head_step_path serves nv_head_step (scale_state = opts = NULL), _scaled (opts = NULL) and _soft.  path == NULL: the
 *   call is handed to the existing symbol (same launches, same bits).  The path-aware kernels are instantiations of their own: what the
 *   existing symbols launch is unchanged.
 * Engine level: nv_vit_drop_path.factors = the whole table.  nv_vit_forward_sd = nv_vit_forward_in + sd (training == 1 only, not the fused
 *   4D input form); nv_vit_backward_sd = nv_vit_backward_attn + sd - it MUST be given the forward's table; nv_vit_train_step_sd =
 *   nv_vit_train_step_ex + sd, every nv_train_hparams form of that call (all fuse_update modes, accumulation, static and dynamic loss scale,
 *   nv_dp_plan, both head routes).  Sites: out-projection of block l f[l, 0], FC2 f[l, 1] (forward, also in the cls-rows form of the last
 *   block); LN2 backward of block l f[l, 0], LN1 backward of block l (l > 0) f[l - 1, 1], the head's backward f[depth - 1, 1].  sd == NULL IS
 *   the existing entry point (same launches, same bits); a wrong struct_size or NULL factors is refused before any launch.  Not in the fp8
 *   training forward and not in nv_vit_backward_tokens. */
#define NV_DROP_PATH_LINEAR 0
#define NV_DROP_PATH_CONSTANT 1
typedef struct nv_vit_drop_path {
  int struct_size;        /* sizeof(nv_vit_drop_path) */
  const float* factors;   /* device [depth][2][B] */
} nv_vit_drop_path;
int nv_drop_path_draw(unsigned long seed, int B, int depth, float rate, int schedule, float* factors, void* stream);
int nv_gemm_bf16_path(int layout, int epi, int M, int N, int K, const void* A, long lda, const void* B, long ldb, void* C,
                      long ldc, const float* bias, const void* aux_in, long ld_aux_in, void* aux_out, long ld_aux_out,
                      int accumulate, float alpha, unsigned long drop_seed, float drop_p, void* stream, const float* path, int path_rows);
int nv_skinny_nt_path(int epi, int R, int N, int K, const void* A, long lda, const void* W, long ldw, const float* bias, const float* resid,
                      long ldr, void* out, long ldo, void* u_out, long ldu, unsigned long drop_seed, float drop_p, void* stream,
                      const float* path, int path_rows);
int nv_ln_bwd_path(const float* dy, long lddy, const float* x, long ldx, const float* mean, const float* rstd, const float* gamma,
                   int M, int d, const float* g_in, float* g_out, long ldg, void* g16, long ldg16, float* dgamma, float* dbeta,
                   float* dcolsum, int accumulate, void* workspace, long ws_bytes, unsigned long drop_seed, float drop_p, void* stream,
                   void* reduce_stream, const float* path, int path_rows);
int nv_head_bwd_path(const float* dlogits, int B, int C, const float* W, const float* x, long row_stride, const float* stats,
                     const float* xh, const float* gamma, int d, int n, float* g, long ldg, void* g16, long ldg16, float* dgamma,
                     float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                     unsigned long drop_seed, float drop_p, int pool_mean, void* stream, const float* path, int path_rows);
int nv_head_step_path(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps, const float* W,
                      const float* bias, int C, const long* labels, float grad_scale, const float* scale_state, const nv_loss_opts* opts,
                      float* xh, float* stats, float* logits, float* loss, float* dlogits, int n, float* g, long ldg, void* g16, long ldg16,
                      float* dgamma, float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                      unsigned long drop_seed, float drop_p, void* stream, const float* path, int path_rows);
int nv_vit_forward_sd(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5,
                      const nv_vit_input* in, const float* params, const void* params16, void* workspace, long ws_bytes,
                      int training, float drop_p, float emb_drop_p, unsigned long drop_seed, float* logits, void* stream,
                      const nv_vit_drop_path* sd);
int nv_vit_backward_sd(const nv_vit_config* cfg, int B, const float* video, const long* strides5, const float* params,
                       const void* params16, void* workspace, long ws_bytes, const float* dlogits, float* grads, void* grads16,
                       int accumulate, int first_stage, int last_stage, float drop_p, float emb_drop_p, unsigned long drop_seed,
                       void* stream, void* aux_stream, int join_aux, int rows_form, const nv_vit_backward_opts* opts,
                       const nv_vit_attn_grad_export* attn_grad, const nv_vit_drop_path* sd);
int nv_vit_train_step_sd(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5, const nv_vit_input* in,
                         float* params, void* params16, float* grads, float* adam_m, float* adam_v, void* workspace, long ws_bytes,
                         const long* labels, float* logits, float* loss, float* dlogits, const nv_train_hparams* hp, const nv_loss_opts* lo,
                         float drop_p, float emb_drop_p, unsigned long drop_seed, void* stream, void* aux_stream, const nv_vit_drop_path* sd);

/* (added within revision 8 - new symbols and one new struct only, nothing existing changes) a regression objective for the head: brain age,
 * a rating, a cognitive score - K = num_classes continuous targets per volume in the place of a class index.
 *   z  = the head's output fp32 [B, K], on the standardised scale;   y = targets fp32 [B, K] on the raw scale; a non-finite y (NaN is the
 *   "missing" marker) makes the cell invalid, m_bk = 0;   mean_k, std_k > 0: device fp32 [K] or NULL for 0 / 1;   w_k >= 0: device fp32 [K]
 *   per-target weight or NULL for ones.
 *     t_bk  = (y_bk - mean_k) / std_k                         (fp32, each operation rounded)
 *     with a mix row (partner p, label lambda l: columns 0 and 3 of nv_mix_params, the columns nv_loss_opts.mix reads)
 *     t_bk  = l t_bk + (1 - l) t_pk,   valid iff both cells are valid
 *     r     = z_bk - t_bk
 *     l(r)  = r^2                                   NV_REG_MSE
 *           = |r|                                   NV_REG_L1      (l'(0) = 0)
 *           = 0.5 r^2 if |r| <= delta, else delta (|r| - 0.5 delta)      NV_REG_HUBER, delta > 0 (F.huber_loss)
 *     D     = sum_bk m_bk w_k                       in double, one fixed order
 *     loss  = sum_bk m_bk w_k l(r_bk) / D
 *     dloss/dz_bk = m_bk w_k l'(r_bk) / D * grad_scale * scale_state[0] (when given)
 *   D == 0 (no observed target in the batch): loss 0 and an all-zero gradient - on purpose not the cross-entropy's NaN: a batch of missing
 *   scores is ordinary data.  A non-finite z in a valid cell propagates (a non-finite loss; a non-finite gradient in every kind), so a dynamic
 *   loss scale sees an overflow as before.  A partner outside [0, B) gives a NaN loss; nothing is read through an unchecked index.  An invalid
 *   cell receives exactly 0.0f.  NV_ERR_ARG before any launch: a wrong struct_size, an unknown kind, delta <= 0 for huber, K > d in the fused
 *   head step.
 * nv_reg_loss: the standalone loss (one launch; dpred may be NULL).  nv_head_step_reg: nv_head_step_path with (targets, nv_reg_opts) in the
 *   place of (labels, nv_loss_opts) - two launches; every workgroup forms D itself (no atomics, no extra launch); one row body with
 *   nv_reg_loss, so head forward + nv_reg_loss + head backward give the same bits; path (may be NULL) as in nv_head_step_path.
 * nv_vit_train_step_reg: nv_vit_train_step_sd with targets fp32 [B, num_classes] for labels and nv_reg_opts for lo; every nv_train_hparams
 *   form of that call (all fuse_update modes, accumulation, static and dynamic loss scale, nv_dp_plan - each rank normalises by its own D -,
 *   the drop-path table or NULL, both head routes).  Backward and update only see dlogits.
 * nv_reg_metrics_update / _finish: validation metrics on the raw scale with no host read per batch.  yhat = (z * std) + mean, the fp32 product
 *   and the fp32 sum each rounded on their own; e = yhat - y over the valid cells.  state: double [K, NV_REG_METRIC_SLOTS], zeroed by the
 *   caller: n, sum e, sum |e|, sum e^2, sum a, sum p, sum a^2, sum p^2, sum a p with a = y - mean, p = yhat - mean (in double).  One
 *   workgroup per target walks the rows in one fixed order: no atomics, the bits reproduce.  finish writes out fp32 [K, 6]: n, MAE, RMSE, bias
 *   (mean e), Pearson r, R^2 = 1 - sum e^2 / sum (y - ybar)^2.  r / R^2 are NaN for n < 2 or zero variance (a sum of squares about the mean
 *   not above 1e-12 of the raw one: the rounding of the double sums); MAE /
 *   RMSE / bias are NaN for n = 0. */
#define NV_REG_MSE 0
#define NV_REG_L1 1
#define NV_REG_HUBER 2
#define NV_REG_METRIC_SLOTS 9
typedef struct nv_reg_opts {
  int struct_size;              /* sizeof(nv_reg_opts): checked */
  int kind;                     /* NV_REG_MSE / NV_REG_L1 / NV_REG_HUBER */
  float delta;                  /* huber's threshold (> 0); ignored by the other kinds */
  const float* mean;            /* device fp32 [K] or NULL (0) */
  const float* std;             /* device fp32 [K], > 0, or NULL (1) */
  const float* weight;          /* device fp32 [K], >= 0, or NULL (ones) */
  const int* mix;               /* device int32 [B, NV_MIX_COLS] rows of nv_mix_params or NULL: partner (column 0) and label lambda (column 3) are read */
} nv_reg_opts;
int nv_reg_loss(const float* pred, const float* target, int B, int K, float grad_scale, const float* scale_state, const nv_reg_opts* opts,
                float* loss, float* dpred, void* stream);
int nv_head_step_reg(const float* x, long row_stride, int B, int d, const float* gamma, const float* beta, float eps, const float* W,
                     const float* bias, int C, const float* targets, float grad_scale, const float* scale_state, const nv_reg_opts* opts,
                     float* xh, float* stats, float* logits, float* loss, float* dlogits, int n, float* g, long ldg, void* g16, long ldg16,
                     float* dgamma, float* dbeta, float* dW, float* dbias, float* dcolsum, int accumulate, void* workspace, long ws_bytes,
                     unsigned long drop_seed, float drop_p, void* stream, const float* path, int path_rows);
int nv_vit_train_step_reg(const nv_vit_config* cfg, int B, const float* video, const long* shape5, const long* strides5, const nv_vit_input* in,
                          float* params, void* params16, float* grads, float* adam_m, float* adam_v, void* workspace, long ws_bytes,
                          const float* targets, float* logits, float* loss, float* dlogits, const nv_train_hparams* hp, const nv_reg_opts* ro,
                          float drop_p, float emb_drop_p, unsigned long drop_seed, void* stream, void* aux_stream, const nv_vit_drop_path* sd);
int nv_reg_metrics_update(const float* pred, const float* target, int B, int K, const float* mean, const float* std, double* state, void* stream);
int nv_reg_metrics_finish(const double* state, int K, float* out, void* stream);

/* (added within revision 8 - new symbols only, nothing existing changes) frozen-feature evaluation: pooled features of the encoder, a fused
 * similarity + top-k search over a feature bank, the weighted k-nearest-neighbour vote and per-segment (per-subject) means.  Every call takes
 * a stream, reads nothing back and uses no atomics; every sum has one fixed order, so results are bit-identical from run to run.
 * nv_pool_features: tokens fp32 [B, n, d], sample b at tokens + b * batch_stride, token row t at + t * row_stride (both in floats, row_stride
 *   >= d) -> row row0 + b of out fp32 [*, ldo] (a preallocated bank is filled in place).  NV_POOL_CLS: row 0, copied.  NV_POOL_MEAN: the mean of
 *   all n rows with the bits of nv_token_mean (fp32 partial sums over the rows t = g, g + 4, ..., g < 4; ((p0 + p1) + (p2 + p3)) / n).
 *   NV_POOL_PATCH_MEAN: the mean of the rows 1 .. n - 1 (n >= 2), summed in double in ascending row order, divided in double, rounded once.
 *   normalize != 0: F.normalize's rule on the pooled fp32 row x: ss = sum x_c^2 in double in ascending column order,
 *   out_c = fp32(x_c / max(sqrt(ss), 1e-12)) formed in double.  d <= 8192.
 * nv_knn_topk: for every row of Q fp32 [Nq, d] (ldq) the k (1 .. 128) rows of bank fp32 [Nb, d] (ldb) with the largest dot product; d, ldq, ldb
 *   multiples of 4, Q and bank 16-byte aligned (as nv_gemm_f32).  INPUTS MUST BE FINITE: a NaN or an infinite similarity has no defined place in
 *   the order.  idx int32 [Nq, k], sim fp32 [Nq, k], best first.  Order: larger sim first; equal sim (compared as floats, -0 == +0) to the
 *   LOWER bank index.  q_group int32 [Nq] and b_group int32 [Nb] (both or neither): bank row j is skipped for query q when q_group[q] >= 0 and
 *   q_group[q] == b_group[j].  With fewer than k eligible rows the remaining slots hold idx -1, sim -inf.  The similarities run on
 *   v_mfma_f32_16x16x4_f32 in fp32 end to end; the Nq x Nb matrix is never written.  splits (0 = automatic, up to 64): the bank's 64-row tiles
 *   are divided over that many workgroups per query tile and a second launch merges their lists under the same order; a dot product's
 *   accumulation order depends on d alone, so every bit of sim and idx is independent of the split count.  More than one split needs a workspace
 *   of nv_knn_topk_workspace_bytes(Nq, Nb, k, splits) bytes (0 for one split); nv_knn_topk_splits returns the count that splits = 0 resolves to
 *   (0 for arguments nv_knn_topk refuses).
 * nv_knn_vote: idx / sim [Nq, kmax] as nv_knn_topk wrote them, the first k <= kmax slots of each row are used.  Weights: NV_KNN_UNIFORM 1, or
 *   NV_KNN_SOFTMAX w_i = expf((sim_i - sim_0) / temperature) (exp(sim / T) made overflow safe: the ratios are unchanged).  A slot is ignored when
 *   idx is outside [0, Nb) (the -1 of an empty slot).  Give labels or targets, not both:
 *   labels int32 [Nb] in [0, C) (any other label: that neighbour is ignored): scores fp32 [Nq, C] = class-wise weight sums / total, summed in
 *   double over i = 0 .. k - 1 in that order; pred int32 [Nq] = arg-max of the double scores, ties to the lower class.  No usable neighbour:
 *   scores 0, pred -1.
 *   targets fp32 [Nb, K]: pred_reg fp32 [Nq, K] = the weighted mean per column over the neighbours whose target is not NaN (the missing-value
 *   marker of nv_reg_loss), in double; NaN when there is none.
 * nv_segment_mean: out[g] (fp32 [G, w], ldo) = the mean of the rows src[order[p]] (fp32 [N, w], lds), offsets[g] <= p < offsets[g + 1], summed
 *   in double in that order and rounded once; an empty segment gives zeros.  order int32 [N] and offsets int32 [G + 1] are DEVICE arrays of a
 *   CSR the caller built on the host; nv_segment_csr_check validates the HOST copies (offsets from 0, non-decreasing, at most N; every order
 *   entry in [0, N)) - NV_ERR_ARG otherwise.  The kernel skips an entry outside [0, N) anyway: nothing is read through an unchecked index.
 *   G <= 65535 per call. */
#define NV_POOL_CLS 0
#define NV_POOL_MEAN 1
#define NV_POOL_PATCH_MEAN 2
#define NV_KNN_UNIFORM 0
#define NV_KNN_SOFTMAX 1
#define NV_KNN_MAX_K 128
int nv_pool_features(const float* tokens, long batch_stride, long row_stride, int B, int n, int d, int mode, int normalize, float* out, long ldo,
                     long row0, void* stream);
int nv_knn_topk_splits(int Nq, int Nb, int splits);
long nv_knn_topk_workspace_bytes(int Nq, int Nb, int k, int splits);
int nv_knn_topk(const float* Q, long ldq, int Nq, const float* bank, long ldb, int Nb, int d, int k, const int* q_group, const int* b_group,
                int splits, int* idx, float* sim, void* workspace, long ws_bytes, void* stream);
int nv_knn_vote(const int* idx, const float* sim, int Nq, int kmax, int k, int weighting, float temperature, int Nb, const int* labels, int C,
                float* scores, int* pred, const float* targets, int K, float* pred_reg, void* stream);
int nv_segment_csr_check(const int* order, const int* offsets, int N, int G);
int nv_segment_mean(const float* src, long lds, int N, int w, const int* order, const int* offsets, int G, float* out, long ldo, void* stream);

/* (added within revision 8 - new symbols and one new struct only, nothing existing changes) a linear probe over the frozen-feature bank: H
 * heads (one per regularisation strength) trained side by side by full-batch Adam steps over ONE read of the features.  Every call takes a
 * stream, reads nothing back and uses no atomics; every sum has one fixed order, so results are bit-identical from run to run.
 *   X fp32 [N, d] (ldx);  z = (x - mean) * rstd, formed in fp32 on load, each operation rounded (mean == NULL: z = x; both or neither).
 *   W fp32 [M, d] dense, b fp32 [M], M = H * C <= NV_PROBE_MAX_M; head h owns the columns [h C, (h + 1) C).  logit = W z + b on
 *   v_mfma_f32_16x16x4_f32, in fp32 end to end.  FEATURES MUST BE FINITE (as nv_knn_topk): a NaN feature reaches every sum it is part of.
 *   Cost of head h: J_h = L_h + (l2_h / 2) |W_h|^2, the bias is not penalised; the L2 term is COUPLED (it is part of the gradient, so the
 *   stationary point is the penalised-likelihood optimum; regression: the ridge solution), not AdamW's decoupled decay.
 *   NV_PROBE_CLASSIFICATION: labels int32 [N]; a row whose label lies outside [0, C) carries no loss and no gradient; p = fp32 softmax over the
 *     head's own C columns (max-subtracted, expf, summed in ascending column order); c_i = class_weight[y_i] (fp32 [C]) or 1;
 *     D = sum_i c_i over the labelled rows;  L_h = sum_i c_i (-log p_i,y_i) / D;  dL_h / dlogit_ik = c_i (p_ik - [k == y_i]) / D.
 *   NV_PROBE_REGRESSION: targets fp32 [N, C] (C = the number of targets), the same targets for every head; t = (y - target_mean_k) /
 *     target_std_k in fp32, each operation rounded (NULL: 0 / 1); a NaN target is missing (the marker of nv_reg_loss) and receives exactly
 *     zero gradient; every target column is a problem of its own: D_k = its count of observed cells, L_h = sum_k sum_i (logit - t)^2 / D_k,
 *     dL_h / dlogit_ik = 2 (logit - t) / D_k.
 *   Nothing observed (D == 0): loss 0 and data gradient 0, not NaN - dW is then l2 W exactly.
 * nv_probe_stats: per column of X (features must be finite unless skip_nan != 0: NaN cells are then left out of sums and counts - the
 *   targets): mean, rstd = 1 / sqrt(var + eps) and (optional) std = sqrt(var) with the population variance, and count fp64 [d] (optional)
 *   = the observed cells.  Two passes (sum, then squared deviations from the fp64 mean), in fp64, each operation rounded: per-column
 *   partials over the row chunks [c NV_PROBE_CHUNK, (c + 1) NV_PROBE_CHUNK) in ascending row order, the chunk partials added in ascending
 *   chunk order, every result rounded once to fp32.  A column whose variance is exactly 0 gets rstd = 0 (the feature drops out instead of
 *   exploding on a query); a column without an observed cell gets mean 0, rstd 0, std 0.  X may be NULL (d = 0) when only denom is wanted.
 *   labels != NULL: denom[0] (fp64) = D of the classification loss above, per-chunk partials in ascending row order, added in ascending chunk
 *   order.  The regression denominators are `count` of the targets under skip_nan.  workspace: nv_probe_stats_workspace_bytes(N, d).
 * nv_probe_grad: one pass over X: logits, per-head loss and dlogits, and the product dlogits^T Z from a 32-row tile of Z staged in LDS for
 *   both products (X is read from memory once).  A workgroup keeps the [M, d] partial of a row chunk in accumulator registers over the
 *   chunk's tiles and writes it once to the workspace; chunk c covers the rows [c NV_PROBE_CHUNK, (c + 1) NV_PROBE_CHUNK) whatever the grid
 *   (max_blocks workgroups walk the chunks; 0 = one per chunk).  A second launch adds the chunk partials in ascending chunk order in fp64
 *   and writes dW[m, j] = fp32(S / D + l2_h W[m, j]) (the product formed in fp64), db[m] = fp32(S_b / D) and loss[h] = fp32(L_h): every bit
 *   is independent of the grid and of the CU count.  denom: fp64 [1] (classification) or fp64 [C] (regression), as nv_probe_stats wrote
 *   them.  d a multiple of 4 in [4, NV_PROBE_MAX_D]; ldx >= d a multiple of 4; X, W, mean, rstd 16-byte aligned; NV_ERR_ARG otherwise.
 *   workspace: nv_probe_grad_workspace_bytes(N, d, M) bytes (0 for arguments nv_probe_grad refuses).
 * nv_probe_step: Adam on W, b and their moments from dW / db in one launch, every fp32 operation rounded on its own (no contraction):
 *     m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  p = p - step_h (m / (sqrt(v) / bc2_sqrt + eps))
 *   with step_h = fp32(lr_h / (1 - b1^t)), bc2_sqrt = fp32(sqrt(1 - b2^t)) and one_minus_b1 / one_minus_b2 formed by the host in fp64 and
 *   passed as floats: bit-equal to the same torch fp32 expressions.
 * nv_probe_predict: Q fp32 [Nq, d] (ldq) -> logits fp32 [Nq, M] (ldl) under mean / rstd, with the bits nv_probe_grad's logits have;
 *   probs (optional, ldp): the fp32 softmax over each head's own C columns. */
#define NV_PROBE_CHUNK 256
#define NV_PROBE_MAX_M 32
#define NV_PROBE_MAX_D 1024
#define NV_PROBE_CLASSIFICATION 0
#define NV_PROBE_REGRESSION 1
typedef struct nv_probe_heads {
  int struct_size;              /* sizeof(nv_probe_heads): checked */
  int H;                        /* heads, >= 1 */
  int C;                        /* columns per head (classes or targets), >= 1; H * C <= NV_PROBE_MAX_M */
  float l2[NV_PROBE_MAX_M];     /* per head, >= 0: read by nv_probe_grad */
  float step[NV_PROBE_MAX_M];   /* per head, lr_h / (1 - b1^t): read by nv_probe_step */
} nv_probe_heads;
long nv_probe_stats_workspace_bytes(int N, int d);
int nv_probe_stats(const float* X, long ldx, int N, int d, int skip_nan, float eps, float* mean, float* rstd, float* std, double* count,
                   const int* labels, int C, const float* class_weight, double* denom, void* workspace, long ws_bytes, void* stream);
long nv_probe_grad_workspace_bytes(int N, int d, int M);
int nv_probe_grad(const float* X, long ldx, int N, int d, const float* mean, const float* rstd, const float* W, const float* b,
                  const nv_probe_heads* heads, int task, const int* labels, const float* class_weight, const float* targets,
                  const float* target_mean, const float* target_std, const double* denom, float* dW, float* db, float* loss, int max_blocks,
                  void* workspace, long ws_bytes, void* stream);
int nv_probe_step(float* W, float* b, const float* dW, const float* db, float* mW, float* vW, float* mb, float* vb, int d,
                  const nv_probe_heads* heads, float beta1, float beta2, float one_minus_b1, float one_minus_b2, float bc2_sqrt, float eps,
                  void* stream);
int nv_probe_predict(const float* Q, long ldq, int Nq, int d, const float* mean, const float* rstd, const float* W, const float* b, int H, int C,
                     float* logits, long ldl, float* probs, long ldp, void* stream);

/* (added within revision 8 - new symbols only, nothing existing changes) classification metrics on the device: what a validation pass of the
 * classifier reports, accumulated with one launch per batch and no host read, an exact one-vs-rest ROC-AUC over a bank of probabilities and
 * the labels of segments (subjects).  Every call takes a stream, reads nothing back and uses no atomics; every sum has one fixed order, so
 * results are bit-identical from run to run.  Limits (NV_ERR_ARG before any launch): 2 <= C <= NV_CLS_MAX_C, 1 <= bins <= NV_CLS_MAX_BINS,
 * B, N >= 1, lds / ldb >= C, state 8-byte aligned, row0 >= 0 and row0 + B <= capacity, N <= NV_CLS_AUC_MAX_N.
 * nv_cls_metrics_update: scores fp32 [B, C] (lds), labels int32 [B], kind NV_CLS_LOGITS | NV_CLS_PROBS.  A row is VALID iff its label lies in
 *   [0, C) (the probe's rule) and all its C scores are finite; any other row adds 1 to `skipped` and carries nothing else.  Per valid row, in
 *   double from the fp32 inputs: pred = the lowest index of the maximal fp32 score (compared as floats: no rounding enters the arg-max);
 *   LOGITS: p_c = exp(z_c - m) / S, m the row maximum, S = sum_c exp(z_c - m) in ascending c, nll = (m + log S) - z_y;  PROBS: p_c = score_c
 *   as given (not renormalised), nll = -log p_y;  brier = sum_c (p_c - [c == y])^2;  conf = p_pred;  bin = min(bins - 1, int(conf * bins))
 *   (a conf below 0 - possible under PROBS only - goes to bin 0).
 *   state: double [nv_cls_metrics_state_doubles(C, bins)], zeroed by the caller; counts are exact integers held in doubles:
 *     [0] n  [1] skipped  [2] sum nll  [3] sum over the calls of (sum nll / n_valid of the call)  [4] calls with a valid row  [5] sum brier
 *     [NV_CLS_STATE_HEAD + t C + p] confusion, true class t x predicted class p
 *     then per bin b: count [bins], sum conf [bins], sum correct [bins].
 *   One workgroup per call: thread t takes the rows t, t + 256, ...; its double partials of nll and brier go through the wave butterfly and
 *   the four waves in order; the confusion cells and the bins are counted from the rows' records in LDS, 256 rows at a time, each cell and
 *   each bin by one owner thread in ascending row order.  The state is updated by plain read-modify-write: the stream orders the calls.
 *   bank_probs fp32 [capacity, C] (ldb) and bank_labels int32 [capacity] (both or neither): rows row0 .. row0 + B - 1 receive float(p_c) and
 *   the label; a skipped row gets zeros and label -1.
 * nv_cls_auc: exact one-vs-rest ROC-AUC per class by counting pairs (the Mann-Whitney statistic, ties counted as a half) - no sort.
 *   probs fp32 [N, C] (ldp), labels int32 [N]; a row whose label lies outside [0, C) (-1 as nv_cls_metrics_update writes it) is not used.
 *     gt_c = #{(i, j): y_i = c, y_j usable and != c, p_ic > p_jc},  eq_c = the same with ==,  AUC_c = (gt_c + eq_c / 2) / (n_pos n_neg).
 *   The comparisons are on the fp32 values, so every count is an exact integer (a NaN cell compares false both ways).  Workgroup (x, y):
 *   rows i in [256 x, 256 x + 256), one per thread - a row is a positive of exactly its own class -, against the j range of split y, streamed
 *   through LDS in tiles (16-byte loads when ldp == C and probs is 16-byte aligned).  A thread counts in 32 bits: its count is at most the rows
 *   of one split <= N <= NV_CLS_AUC_MAX_N = 2^20 < 2^31 (enforced); the per-class totals of a workgroup (64-bit) go to the workspace of
 *   nv_cls_auc_workspace_bytes(N, C, splits) bytes and a second launch adds them in 64 bits.  splits: 0 = automatic, up to
 *   NV_CLS_AUC_MAX_SPLITS; the counts do not depend on it, on the grid or on the CU count.  out: double [C, NV_CLS_AUC_COLS] = auc, n_pos,
 *   n_neg, gt, eq (all exact in a double: gt <= N^2 / 4 <= 2^38); auc is NaN where a class has no positive or no negative row.
 *   The cost is quadratic: measured 1.35 ms at N = 78 820 (MI355X), i.e. about 0.25 s at NV_CLS_AUC_MAX_N - the limit is set by that run time,
 *   not by the counters: larger banks belong to a sort.
 * nv_segment_labels: out[g] (int32 [G]) = labels[order[offsets[g]]], the label of the segment's first row (order / offsets: the device CSR
 *   of nv_segment_mean); an empty segment gets -1.  mixed (int32 [1], overwritten): the number of segments that hold a row whose label is >= 0
 *   and differs from the segment's.  One workgroup; entries of order outside [0, N) are skipped.
 * nv_cls_metrics_finish: state (+ auc, the table of nv_cls_auc, or NULL) -> out fp32 [nv_cls_metrics_table_floats(C)]:
 *     [0 .. NV_CLS_SCALARS): n, skipped, accuracy, balanced_accuracy (mean recall over the classes with support), macro_f1 (mean of
 *       2TP / (2TP + FP + FN) over the classes where that denominator is not 0), nll (mean over rows), val_loss (mean over the calls of the
 *       calls' means), brier, ece = sum_b |sum correct_b - sum conf_b| / n, macro_auc (mean over the classes whose AUC is defined)
 *     then [C, NV_CLS_CLASS_COLS]: support, recall, precision, f1, auc;  then the confusion matrix [C, C] as fp32 - exact up to 2^24 rows.
 *   Undefined quantities are NaN, never 0: everything but n / skipped for n = 0, recall without support, precision without a prediction, f1
 *   with a zero denominator, an AUC with one side empty or without a table, a mean over no class. */
#define NV_CLS_LOGITS 0
#define NV_CLS_PROBS 1
#define NV_CLS_MAX_C 64
#define NV_CLS_MAX_BINS 64
#define NV_CLS_STATE_HEAD 6
#define NV_CLS_SCALARS 10
#define NV_CLS_CLASS_COLS 5
#define NV_CLS_AUC_COLS 5
#define NV_CLS_AUC_MAX_N (1 << 20)
#define NV_CLS_AUC_MAX_SPLITS 256
long nv_cls_metrics_state_doubles(int C, int bins);
long nv_cls_metrics_table_floats(int C);
int nv_cls_metrics_update(const float* scores, long lds, const int* labels, int B, int C, int bins, int kind, double* state, float* bank_probs,
                          long ldb, int* bank_labels, long row0, long capacity, void* stream);
int nv_cls_auc_splits(int N, int C, int splits);
long nv_cls_auc_workspace_bytes(int N, int C, int splits);
int nv_cls_auc(const float* probs, long ldp, const int* labels, int N, int C, int splits, double* out, void* workspace, long ws_bytes,
               void* stream);
int nv_segment_labels(const int* labels, int N, const int* order, const int* offsets, int G, int* out, int* mixed, void* stream);
int nv_cls_metrics_finish(const double* state, int C, int bins, const double* auc, float* out, void* stream);

/* (added within revision 8 - new symbols only, nothing existing changes) group-level permutation tests with the maximum statistic (Nichols &
 * Holmes): where are N maps fp32 [N, V] (ldx; one per subject) consistently non-zero (one sample, sign flips), or where do two groups differ
 * (two samples, label permutation, pooled-variance Student t), with the family-wise error controlled over all voxels.  Every call takes a
 * stream, reads nothing back and uses no atomics; every count is an exact integer and no output bit depends on the grid, the split count or
 * the CU count.  Limits (NV_ERR_ARG before any launch): 2 <= N <= NV_PERM_MAX_N (3 and both groups non-empty for two samples),
 * 1 <= R <= NV_PERM_MAX_R, V >= 1, ldx >= V, splits in [0, NV_PERM_MAX_SPLITS] (0 = automatic), exact enumeration only for one sample with
 * R = 2^N <= NV_PERM_MAX_R.
 * The statistic.  Per voxel, in double over the subjects in ascending order (every product and sum rounded on its own): T = sum x_i,
 *   Q = sum x_i^2, and for two samples S_A = the sum over the subjects of label 1.
 *     one sample:   a = 0,           c = 1 / sqrt(N Q),                     u = (S - a) c,  t = u sqrt((N - 1) / (1 - u^2))
 *     two samples:  a = n_A T / N,   c = 1 / sqrt(n_A n_B SS / N), SS = Q - T^2 / N,        t = u sqrt((N - 2) / (1 - u^2))
 *   with S = sum_i m_i x_i for a row m of the design (signs +-1; 0/1 marks of group A = label 1, so t > 0 where group 1 has the larger
 *   mean).  t is strictly increasing in u on [-1, 1]; the permutation loop works on u alone.  a and c are rounded to fp32 once; in the loop
 *   u = float(float(S - a) * c) with S accumulated in fp32 on the matrix unit, clamped to [-1, 1].  The statistic is |u| (NV_PERM_TAIL_TWO),
 *   u (_GREATER) or -u (_LESS); ties count (>=).
 * A voxel is INVALID when it lies outside mask (uint8 [V], 0 = outside; NULL = no mask), holds a non-finite value, has Q == 0 (one sample)
 *   or SS <= 0 (two samples), or its c does not fit fp32: a = c = 0, t and both p-values NaN, both counts 0, counted in n_invalid, in no
 *   maximum.  A voxel whose values are all equal and not zero has t = +-inf in the one-sample test.
 * nv_perm_design: M fp32 [R, Npad], Npad = N rounded up to 4, pad columns 0.  Row 0 is the observed labelling (all +1; m_i = [labels_i == 1]).
 *   One sample, exact (R = 2^N): subject i of row r is -1 iff bit i of r is set.  One sample, random, r >= 1: -1 iff bit (i & 63) of
 *   nv_hash64(seed ^ 0x5045524D31, r ceil(N / 64) + (i >> 6)) is set.  Two samples, r >= 1: keys nv_hash64(seed ^ 0x5045524D32, r N + i);
 *   subject i is in group A iff its ascending rank among the row's keys is below n_a (equal keys: the lower index first).  labels: device
 *   int32 [N] (two samples only; n_a must be their number of ones).  nv_hash64 as for nv_augment_params.
 * nv_perm_stats: a, c, t fp32 [V] (t: the observed statistic from the double u, rounded once) and n_invalid int32 [1].
 * nv_perm_maxstat: P = M X is never written.  A workgroup stages the [Npad, NV_PERM_TILE_V] slab of its voxel tile in LDS once and walks its
 *   rows of M (from L2) in tiles of NV_PERM_TILE_R on v_mfma_f32_16x16x4_f32 - fp32 operands on purpose: the comparisons stat_r >= stat_0
 *   decide the p-values.  Fused epilogue: the row maxima of the tile's valid voxels go to a table [R, tiles of V], the per-voxel counts
 *   #{r: stat_r(v) >= stat_0(v)} stay in registers over the whole walk (stat_0 comes from the same product of row 0, so the same bits).
 *   The rows are split over the grid's second dimension (splits); the split partials of the counts are integers, added in split order.
 * nv_perm_finish (two launches): max_stat fp32 [R] (-0 as +0), max_t fp32 [R] = the transform of max_stat, formed in double;
 *   count_unc / count_fwe int32 [V] (count_fwe[v] = #{r: max_stat[r] >= stat_0(v)}, R V comparisons); p = float(count / R), row 0 counted,
 *   so p >= 1 / R; critical_t fp32 [n_alphas] = the transform of the k-th smallest row maximum, k = nv_perm_rank(alpha, R) =
 *   R - floor(alpha R + 1e-9), i.e. the smallest m with #{r: max_r <= m} >= ceil((1 - alpha) R), found by counting (alphas: HOST doubles in
 *   (0, 1), at most NV_PERM_MAX_ALPHAS).  c: the array of nv_perm_stats (validity).
 * The workspace (nv_perm_workspace_bytes(R, V, splits) bytes, 16-byte aligned) is shared by nv_perm_stats, nv_perm_maxstat and
 *   nv_perm_finish of one test, called in that order on one stream with the same R, V and splits. */
#define NV_PERM_ONE_SAMPLE 0
#define NV_PERM_TWO_SAMPLE 1
#define NV_PERM_TAIL_TWO 0
#define NV_PERM_TAIL_GREATER 1
#define NV_PERM_TAIL_LESS 2
#define NV_PERM_MAX_N 256
#define NV_PERM_MAX_R (1 << 20)
#define NV_PERM_MAX_SPLITS 256
#define NV_PERM_MAX_ALPHAS 8
#define NV_PERM_TILE_V 64
#define NV_PERM_TILE_R 64
int nv_perm_splits(int R, int V, int splits);
long nv_perm_workspace_bytes(int R, int V, int splits);
int nv_perm_rank(double alpha, int R);
int nv_perm_design(int kind, int N, int n_a, const int* labels, int R, int exact, unsigned long seed, float* M, void* stream);
int nv_perm_stats(const float* X, long ldx, int N, int V, int kind, int n_a, const int* labels, const unsigned char* mask, float* a, float* c,
                  float* t, int* n_invalid, void* workspace, long ws_bytes, void* stream);
int nv_perm_maxstat(const float* X, long ldx, int N, int V, const float* M, int R, const float* a, const float* c, int tail, int splits,
                    void* workspace, long ws_bytes, void* stream);
int nv_perm_finish(int kind, int N, int R, int V, int splits, const float* c, const double* alphas, int n_alphas, float* max_stat, float* max_t,
                   int* count_unc, int* count_fwe, float* p_unc, float* p_fwe, float* critical_t, void* workspace, long ws_bytes, void* stream);

/* diagnostic: where do the workgroups of a grid run?  out u32 [blocks][2] = (HW_REG_HW_ID, HW_REG_XCC_ID) of each workgroup, which then
 * holds its CU for hold_us microseconds (threads per workgroup / dynamic LDS bytes shape its footprint).  Used to read the CU set of a
 * CU-masked stream (hipExtStreamCreateWithCUMask) and the XCD placement the 1-D grids rely on for speed. */
int nv_cu_census(unsigned* out, int blocks, int threads, int lds_bytes, int hold_us, void* stream);

/* ABI revision of this header: bumped whenever a struct gains a field or an entry point changes its argument list (the list is in
 * INTEGRATION.md "ABI revisions").  A caller built against revision R must refuse a library whose nv_abi_version() != R. */
#define NV_ABI_VERSION 8
int nv_abi_version(void);
/* dst[b .. b + len) = bf16(src[b .. b + len)) for `count` element ranges (HOST arrays begins / lens; any count) */
int nv_cast_ranges_bf16(const float* src, void* dst, const long* begins, const long* lens, int count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NEUROVIT_HIP_H */
