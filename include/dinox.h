/* dinox.h -- C ABI of libdinox_hip.so, the MI355X (gfx950) kernel library for the DINO-X hot path.
 *
 * The reference (timlawrenz/DINO-X) has no FFI or operator registry: every op on its hot path is
 * an ATen call made from Python.  The drop-in seam is therefore the Python
 * module surface (zoo.arch / zoo.hub / zoo.encode / scripts/phase5_big_run.py), and this header is
 * the boundary *underneath* it: one entry point per ATen call sequence that the reference issues
 * on the path.  Each entry cites the reference lines it replaces (paths relative to the reference
 * checkout).  INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions (all entries):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host";
 *   - the caller allocates and owns every buffer, including workspaces (sizes via *_ws_bytes);
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no entry synchronises, allocates or frees, so every entry is hipGraph-capturable;
 *   - return 0 on success, a negative DINOX_E* code on bad arguments, or the positive
 *     hipError_t of a failed launch; the message is kept per thread for dinox_last_error();
 *   - re-entrant from any host thread (autograd's backward thread included): no mutable globals;
 *   - dtype codes: activations/weights may be fp32 ("parity mode", exact-fp32 MFMA / VALU) or
 *     bf16 ("throughput mode": bf16 MFMA operands, fp32 accumulation); the residual stream,
 *     LayerNorm statistics, softmax, losses, gradients of parameters and optimiser state are
 *     always fp32, mirroring what torch.autocast does on the reference path.
 */
#ifndef DINOX_H
#define DINOX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DINOX_ABI_VERSION 3   /* 3: + dinox_block_forward / _backward, dinox_gemm_timer_*, dinox_retrieval_* (later also dinox_retrieval_rank_windowed*, dinox_row_dots), dinox_knn_*, dinox_gram_*, dinox_softmax_probe*, dinox_ntxent_* (later also dinox_ntxent_*_rect), dinox_normalize_bwd, dinox_mae_*, dinox_attention_rows*, dinox_attention_rollout_step*, dinox_ibot_*, dinox_gather_rows, dinox_scatter_add_rows, dinox_seg_*, dinox_surface_*, dinox_cc_*, dinox_cc3d_*, dinox_surface3d_* (all additive: no entry
                               * of an earlier library changed, so the number callers test, dinox_version() == 3, stays; probe the symbol
                               * to learn whether a given build has the later additions) */

/* dtype codes */
#define DINOX_F32 0
#define DINOX_BF16 1
#define DINOX_U16 2   /* source planes of dinox_encode_preprocess only */
#define DINOX_I16 3

/* error codes (negative); positive returns are hipError_t values */
#define DINOX_OK 0
#define DINOX_EINVAL (-1)      /* bad argument (null pointer, non-positive size, ...) */
#define DINOX_EUNSUPPORTED (-2) /* combination not implemented (e.g. bf16 GEMM with transA!=transB) */
#define DINOX_EALIGN (-3)      /* pointer / leading dimension not aligned as the bf16 path needs */

int dinox_version(void);
/* Human-readable description of the last failure on the calling thread ("" if none). */
const char* dinox_last_error(void);
/* 1 if device 0 is a gfx950 part and kernels can launch, 0 otherwise (host query, no launch). */
int dinox_device_ok(void);

/* ------------------------------------------------------------------------------------------
 * GEMM with fused epilogue -- replaces nn.Linear / nn.Conv2d(k=s=patch) / torch.bmm:
 *   zoo/arch.py:46 (qkv), :53 (proj), :76 (fc1 -> GELU -> fc2), :216 (patch_embed),
 *   :253-255 (head), scripts/phase5_big_run.py:727 (Gram bmm), and their autograd backward.
 *
 *   C[b][m][n] = epilogue( alpha * sum_k A(b,m,k) * B(b,n,k) )
 *   transA = 0: A stored [M][K] (K contiguous, lda >= K);  1: A stored [K][M] (lda >= M)
 *   transB = 0: B stored [N][K] (nn.Linear weight layout, ldb >= K);  1: B stored [K][N]
 *   in_dtype applies to A and B; out_dtype to C and aux.  bf16 inputs support (0,0) "NT" and
 *   (1,1) "TN" only (pre-transposed bf16 weight copies make every hot-path product one of them).
 *
 * epilogue bits (applied in this order):
 *   BIAS      acc += bias[n]                       (fp32 [N])
 *   GELU      if aux: aux = acc (pre-activation, out_dtype, ld = ldaux); acc = gelu_erf(acc)
 *   DGELU     acc *= gelu_erf'(aux[m][n])          (aux read, out_dtype)
 *   RESIDUAL  acc += residual[m][n]                (fp32, ld = ldr)
 *   ACCUM     C += acc instead of C = acc          (fp32 C only)
 *
 * Addressing (every kernel, tests/test_gemm_contract_gpu.py holds each of them to it):
 *   A(b,m,k) = A[b strideA + m lda + k]  (transA = 1: A[b strideA + k lda + m]);  B alike;  C[b strideC + m ldc + n].
 *   Leading dimensions may exceed the width; what lies between the width and the leading dimension, between batch items and
 *   around the operands is never used (inputs) and never written (C, aux, colsum) -- vector stores included.
 *   strideA / strideB = 0 shares the operand between the batch items; strideC must keep the items of C apart.
 *   aux and residual have NO stride field: item b starts M ldaux / M ldr elements after item b - 1, i.e.
 *   aux[b M ldaux + m ldaux + n], residual[b M ldr + m ldr + n] (rows of all items at one pitch, as a [batch M][N] matrix).
 *   bias is shared by the batch items.  alpha scales the product only (before BIAS), never colsum.
 *   Alignment never changes the result, only the kernel: the bf16 MFMA kernels need A, B on 16 bytes and lda, ldb, strideA,
 *   strideB multiples of 8; those that store by 16-byte vectors also C, aux, residual, bias on 16 bytes, rows of C and aux of
 *   a multiple of 16 bytes and ldr a multiple of 4.  Anything else runs on a kernel that takes it (in the end gemm_f32, which
 *   multiplies the bf16 values in exact fp32); dinox_gemm_kernel_name tells which.
 * ------------------------------------------------------------------------------------------ */
#define DINOX_EPI_BIAS 1
#define DINOX_EPI_GELU 2
#define DINOX_EPI_DGELU 4
#define DINOX_EPI_RESIDUAL 8
#define DINOX_EPI_ACCUM 16
#define DINOX_EPI_AUXGRAD 32   /* modifies GELU: aux receives gelu_erf'(pre-activation) instead of the pre-activation;
                                * modifies DGELU: acc *= aux (aux already holds the derivative).  Saves the
                                * transcendental work of the backward epilogue: forward evaluates erf/exp once for both. */

typedef struct dinox_gemm_args {
  const void* A;
  const void* B;
  void* C;
  int64_t M, N, K;
  int64_t lda, ldb, ldc;
  int64_t batch;                       /* >= 1 */
  int64_t strideA, strideB, strideC;   /* elements between batch items (0 = shared operand) */
  int32_t transA, transB;
  int32_t in_dtype, out_dtype;
  int32_t epilogue;
  float alpha;
  const float* bias;
  const float* residual;
  int64_t ldr;
  void* aux;
  int64_t ldaux;
  float* colsum;                       /* optional, transA = 1 only: colsum[m] = sum_k A(m,k) (overwritten; added to
                                        * under ACCUM, like C) -- the bias
                                        * gradient sum_rows(dY) rides along the dW = dY^T X product that already streams dY */
  void* ws;                            /* optional workspace of dinox_gemm_ws_bytes() bytes; its contents need not be initialised.  With it a
                                        * split-K product (the dW = dY^T X products, K = every token of the batch) runs as TWO launches on
                                        * the caller's stream: the split kernel stores its partial tiles there by plain stores, a reduction
                                        * kernel then sums them in split order into C -- no counters, no atomics: results are
                                        * bit-reproducible from run to run, and 33 MB of memory-side atomics per launch (1.3 TB/s on this
                                        * part) become plain stores (6 TB/s).  NULL: fp32 atomics into C (one launch, not reproducible).
                                        * One product at a time per workspace; reuse in stream order is fine.  (NT products ignore it,
                                        * except that tools/pp_stamps.py hands the ping-pong kernels a diagnostic stamp buffer here.) */
} dinox_gemm_args;

int dinox_gemm(const dinox_gemm_args* args, void* stream);
/* Bytes of workspace that make this product deterministic (0: it needs none / cannot use one: only a split-K TN product with ONE
 * contiguous fp32 result -- batch = 1, ldc = N, epilogue empty or ACCUM -- has a two-stage reduction; with ldc != N or batch > 1
 * the partial sums meet through fp32 atomics under ACCUM, and without ACCUM, where C would have to be zeroed first and is not
 * contiguous, the product runs as one split). */
int64_t dinox_gemm_ws_bytes(const dinox_gemm_args* args);
/* Name of the device kernel dinox_gemm would launch for these arguments ("gemm_bf16_nt", "gemm_bf16_nt_glds", "gemm_bf16_nt_areg",
 * "gemm_bf16_nt_pp", "gemm_bf16_nt_pp128", "gemm_bf16_nt_pp384", "gemm_bf16_tn", "gemm_bf16_tn_dma", "gemm_bf16_tn_big",
 * "gemm_f32"); host-only query used by bench.py to attribute per-launch timings and by the tests to see that a case ran on the
 * kernel it is about.  Static string. */
const char* dinox_gemm_kernel_name(const dinox_gemm_args* args);

/* out[n] (+)= sum_m x[m][n]   -- bias gradients (autograd of nn.Linear bias, zoo/arch.py:40-41,71-73). */
int dinox_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ldx, int dtype, int accumulate,
                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Linear + residual + LayerNorm in one launch (bf16 mode, model width N = 384) -- replaces, inside a pre-norm block
 * (zoo/arch.py:94-97), the tail of one sub-block and the head of the next:
 *     x_out = residual + a W^T + bias          (proj :53 / fc2 :76 and the residual add :95 / :96; fp32 residual stream)
 *     y     = LayerNorm(x_out; gamma, beta)    (the following norm2 / next block's norm1 / final norm :96,:95,:237)
 * a: [M,K] bf16, w: [N,K] bf16 (nn.Linear layout), bias [N] or NULL, residual [M,N] fp32 or NULL; x_out [M,N] fp32;
 * y [M,N] in y_dtype (DINOX_BF16 when it feeds the next GEMM, DINOX_F32 for the model's final norm); mean, rstd [M]
 * (biased variance, what dinox_layernorm_bwd consumes).  One workgroup owns 128 complete rows, so the residual stream is
 * not read back by a separate LayerNorm launch.  dinox_linear_residual_ln_ok tells whether the fused kernel takes a shape
 * (N == 384, K % 32 == 0); otherwise use dinox_gemm + dinox_layernorm_fwd.
 * ------------------------------------------------------------------------------------------ */
int dinox_linear_residual_ln_ok(int64_t M, int N, int K);
int dinox_linear_residual_ln(const void* a, const void* w, const float* bias, const float* residual, float* x_out,
                             const float* gamma, const float* beta, float eps, void* y, int y_dtype, float* mean,
                             float* rstd, int64_t M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm -- replaces nn.LayerNorm(D), eps 1e-5, affine (zoo/arch.py:89,91,126,187; calls :95,96,237).
 * x is the fp32 residual stream; y is written in out_dtype (bf16 when it only feeds a GEMM).
 * bwd: dx = (dx_add ? dx_add : 0) + LN'(dy)  -- dx_add is the gradient arriving over the skip connection of the
 *      pre-norm block (may be NULL, may alias dx);  dw, db overwritten, or added to when accumulate != 0 (gradient
 *      arena).  ws: dinox_layernorm_bwd_ws_bytes(rows, dim) bytes.
 *      dx_lowp (optional, may be NULL): bf16 copy of the final dx -- the residual-stream gradient is the
 *      dY operand of the next backward GEMMs, which autocast rounds to bf16 at that point as well.
 * ------------------------------------------------------------------------------------------ */
int dinox_layernorm_fwd(const float* x, const float* w, const float* b, void* y, float* mean, float* rstd,
                        int64_t rows, int dim, float eps, int out_dtype, void* stream);
int64_t dinox_layernorm_bwd_ws_bytes(int64_t rows, int dim);
int dinox_layernorm_bwd(const void* dy, const float* x, const float* w, const float* mean, const float* rstd,
                        float* dx, const float* dx_add, void* dx_lowp, float* dw, float* db, void* ws,
                        int64_t rows, int dim, int dy_dtype, int accumulate, void* stream);
/* The input-gradient product in front of a LayerNorm and that LayerNorm's backward as ONE launch (width N = 384, bf16 operands;
 * backward of zoo/arch.py:95-96 with :46 / :75): dy = a w^T (a [M,K], w [384,K] = W^T of the Linear, rounded to bf16 as dinox_gemm
 * would hand it over), then dinox_layernorm_bwd's contract on it -- dx equal to the two calls to the last bit.  ws as dinox_layernorm_bwd. */
int dinox_linear_ln_bwd_ok(int64_t M, int N, int K);
int dinox_linear_ln_bwd(const void* a, const void* w, const float* x, const float* gamma, const float* mean, const float* rstd,
                        float* dx, const float* dx_add, void* dx_lowp, float* dgamma, float* dbeta, void* ws, int64_t M, int N,
                        int K, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * Multi-head self-attention core -- replaces the reshape/permute/unbind +
 * F.scaled_dot_product_attention + transpose/reshape of zoo/arch.py:45-52 (scale 1/sqrt(d), no mask).
 * qkv is the packed output of the qkv Linear, [B][N][3][heads][d]; o is [B][N][heads*d];
 * lse is the per-row log-sum-exp of the scaled scores, [B][heads][N] fp32 (saved for backward).
 * bwd recomputes P from lse (flash style); dqkv has the layout of qkv; ws: dinox_attention_bwd_ws_bytes() bytes.
 * ------------------------------------------------------------------------------------------ */
int dinox_attention_fwd(const void* qkv, void* o, float* lse, int B, int N, int heads, int d, int dtype,
                        void* stream);
/* Rows of a materialised fp32 score matrix [rows][n] (rows = (image, query) pairs of one head; row r's log-sum-exp lives at
 * lse[(r / rows_per_image) * lse_image_stride + r % rows_per_image], i.e. inside the [B][heads][N] tensor of the calls above):
 *   softmax_rows:     s <- softmax(s) in place, lse written;
 *   softmax_bwd_rows: s <- p = exp(s - lse), dp <- ds = p * (dp - sum_j p_j dp_j) * scale, both in place.
 * Used by the fp32 parity mode, which runs full-size attention as batched exact-fp32 products around these two. */
int dinox_softmax_rows(float* s, float* lse, int64_t rows, int n, int rows_per_image, int64_t lse_image_stride, void* stream);
int dinox_softmax_bwd_rows(float* s, float* dp, const float* lse, float scale, int64_t rows, int n, int rows_per_image,
                           int64_t lse_image_stride, void* stream);
int64_t dinox_attention_bwd_ws_bytes(int B, int N, int heads);
int dinox_attention_bwd(const void* d_o, const void* qkv, const void* o, const float* lse, void* dqkv, void* ws,
                        int B, int N, int heads, int d, int dtype, void* stream);
/* north_star's "fused QKV projection + multi-head attention" as ONE launch, for passes that keep nothing for a backward (the teacher
 * of a training step, encode()): qkv = x wqkv^T + bias (zoo/arch.py:46 `self.qkv`) and softmax(q k^T / sqrt(d)) v (:47-52) per
 * (image, head) without the packed qkv tensor ever reaching HBM.  bf16: x [B*N][D], wqkv [3*heads*d][D], bias fp32 [3*heads*d] or NULL
 * -> o [B*N][heads*d].  qkv_out ([B*N][3*heads*d]) and lse ([B*heads][N] fp32) are optional outputs (NULL: not written).
 * dinox_qkv_attention_ok: 1 inside the kernel's envelope (d = 64, 193 <= N <= 224, D % 32 == 0); outside it the entry returns
 * DINOX_EUNSUPPORTED and the caller composes dinox_gemm + dinox_attention_fwd.  Measured on MI355X it is on a par with those two
 * launches at ViT-S and slower at ViT-L: dinox_block_forward uses it only when asked to (qkv == NULL). */
int dinox_qkv_attention_ok(int B, int N, int heads, int d, int D);
int dinox_qkv_attention_fwd(const void* x, const void* wqkv, const float* bias, void* o, void* qkv_out, float* lse, int B, int N,
                            int heads, int d, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch unfold + token assembly -- replaces the im2col half of nn.Conv2d(3,D,k=p,s=p) and
 * flatten/transpose/cat/+pos_embed/+scale_embed/cat of zoo/arch.py:216-229.
 * unfold: x fp32 NCHW [V][3][H][W] -> u [V*P][3*p*p] in out_dtype (the A operand of the patch GEMM;
 *         computed once per step and shared by student and teacher, which see the same batch).
 * assemble fwd: tokens[v][0] = cls + pos[0] (+scale[v]);  tokens[v][1+i] = patches[v][i] + pos[1+i] (+scale[v]);
 *               tokens[v][1+P+r] = registers[r].   tokens is the fp32 residual stream [V][N][D].
 * assemble bwd: dpatches (dtype) for the patch GEMM's dW/db; dcls, dpos, dregs reduced over the batch;
 *               dscale[v] = sum over the 1+P body tokens (NULL when not scale-aware).
 * ------------------------------------------------------------------------------------------ */
int dinox_patch_unfold(const float* x, void* u, int V, int H, int W, int patch, int out_dtype, void* stream);
/* The same with rows of ld >= 3 p^2 elements, the tail zero-filled (patch sizes whose 3 p^2 is no multiple of 8: the operand of the
 * MFMA bf16 products is padded; the weight operand gets zero columns to match). */
int dinox_patch_unfold_ld(const float* x, void* u, int V, int H, int W, int patch, int ld, int out_dtype, void* stream);
int dinox_tokens_fwd(const void* patches, const float* cls, const float* pos, const float* registers,
                     const float* scale, float* tokens, int V, int P, int R, int D, int patches_dtype,
                     void* stream);
int dinox_tokens_bwd(const float* dtokens, void* dpatches, float* dcls, float* dpos, float* dregs,
                     float* dscale, int V, int P, int R, int D, int patches_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * ScaleEmbedding -- replaces Linear(3,h) -> GELU -> Linear(h,D) -> LayerNorm(D) (zoo/arch.py:119-140).
 * All fp32 (V rows only).  fwd saves hpre [V][h], e [V][D] (pre-LN), mean/rstd [V] for backward.
 * bwd overwrites every parameter gradient and dspacing [V][3] (may be NULL).
 * ------------------------------------------------------------------------------------------ */
int dinox_scale_embed_fwd(const float* spacing, const float* w0, const float* b0, const float* w2,
                          const float* b2, const float* lnw, const float* lnb, float* out, float* hpre,
                          float* e, float* mean, float* rstd, int V, int h, int D, float eps, void* stream);
int64_t dinox_scale_embed_bwd_ws_bytes(int V, int h, int D);   /* 0 for every size dinox_scale_embed_bwd refuses */
int dinox_scale_embed_bwd(const float* dout, const float* spacing, const float* w0, const float* w2,
                          const float* lnw, const float* hpre, const float* e, const float* mean,
                          const float* rstd, float* dw0, float* db0, float* dw2, float* db2, float* dlnw,
                          float* dlnb, float* dspacing, void* ws, int V, int h, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * DINO centring/sharpening cross-entropy -- replaces DINOLoss.forward/update_center
 * (scripts/phase5_big_run.py:686-720).  s, t: [2B][K] fp32 logits, rows [view1; view2].
 *   loss[0] = (1/2B) sum_i -sum_k softmax((t[pair(i)]-center)/tt)[k] * log_softmax(s[i]/ts)[k],
 *   pair(i) = (i+B) mod 2B;   ds = grad_scale * dloss/ds (NULL to skip);  row_loss: [2B] workspace.
 * colmean: out[k] = mean_i t[i][k]  (the batch centre; all-reduced across ranks under DP before
 * dinox_center_ema applies  center = center*m + mean*(1-m), phase5_big_run.py:689-690).
 * ------------------------------------------------------------------------------------------ */
int dinox_dino_ce(const float* s, const float* t, const float* center, float student_temp, float teacher_temp,
                  float grad_scale, float* loss, float* ds, float* row_loss, int rows2B, int K, void* stream);
/* Multi-crop form (an extension: the reference trains on 2 global views only).  s: [n_views][B][K] student logits, view-major,
 * the first n_global views being the ones the teacher saw; t: [n_global][B][K].  Every pair (teacher view q, student view
 * v != q) contributes mean_b of the cross-entropy above; loss[0] = their average over the n_global*(n_views-1) pairs.
 * n_global = n_views = 2 is dinox_dino_ce.  ws: (n_views + 2 n_global) * B floats. */
int dinox_dino_ce_multi(const float* s, const float* t, const float* center, float student_temp, float teacher_temp,
                        float grad_scale, float* loss, float* ds, float* ws, int B, int n_global, int n_views, int K,
                        void* stream);
int dinox_colmean(const float* t, float* out, int rows, int K, void* stream);
int dinox_center_ema(float* center, const float* batch_mean, float momentum, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sinkhorn-Knopp teacher centring (DINOv2/v3; an extension, the reference keeps the EMA centre only) -- csrc/sinkhorn.hip.
 * t: [R][K] fp32 teacher logits, row-major; z[i][k] = t[i][k] / tau.  The published loop (exp(z)^T normalised by its sum, then n_iters
 * times: over prototypes, over samples) ends on rows  Q[i][:] = softmax_k((t[i][k] - c[k]) / tau)  with  c = -tau b_n,
 *     a_0 = 0,   b_n[k] = -log sum_i exp(z[i][k] + a_{n-1}[i]),   a_n[i] = -log sum_k exp(z[i][k] + b_n[k]),
 * which is the form dinox_dino_ce / dinox_dino_ce_multi take their targets in: c goes where the EMA centre goes.
 *   sk_col_lse: out[k] = out_scale * log sum_i exp(t[i][k] * inv_temp + a[i])   (a NULL: zeros);  ws: 2 * ceil(R/32) * K floats
 *               (dinox_sk_ws_floats(R, K) covers it), per-chunk (max, sum) partials that a second launch meets in chunk order.
 *   sk_row_lse: out[i] = out_scale * log sum_k exp(t[i][k] * inv_temp + b[k])   (b NULL: zeros).
 *   sk_center:  the 2 n_iters - 1 passes of one rank, center_out[k] = c[k];  ws: dinox_sk_ws_floats(R, K) floats
 *               (= 2 * ceil(R/32) * K + K + R).
 * out_scale = -1 turns a pass into the next pass's a / b; under data parallelism a column pass over the global batch is sk_col_lse on
 * the local rows, an all-gather of the K results into [world][K], and sk_col_lse on that matrix (inv_temp 1, a NULL).
 * fp32, max-shifted (no exp of an unshifted logit), fixed reduction order, no atomics: a pure function of the inputs; finite inputs
 * give finite outputs.  float4 loads when K % 4 == 0 and t (and ws, b) are 16-byte aligned, scalar kernels otherwise.  R < 1, K < 1,
 * n_iters < 1, teacher_temp <= 0, a null pointer, or R > 65535 * 32 in a column pass return DINOX_EINVAL before any launch.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_sk_ws_floats(int R, int K);
int dinox_sk_col_lse(const float* t, const float* a, float inv_temp, float out_scale, float* out, float* ws, int R, int K,
                     void* stream);
int dinox_sk_row_lse(const float* t, const float* b, float inv_temp, float out_scale, float* out, int R, int K, void* stream);
int dinox_sk_center(const float* t, float teacher_temp, int n_iters, float* center_out, float* ws, int R, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gram anchoring -- replaces compute_gram_matrix / compute_gram_anchoring_loss
 * (scripts/phase5_big_run.py:723-739): tokens 1..N-1 (registers included), F.normalize eps 1e-12,
 * G = Xh Xh^T, mse_loss mean.  The Gram products themselves go through dinox_gemm (batched);
 * these entries are the fused pieces around it:
 *   normalize: cat[v][t][0:D] = s_hat, cat[v][t][D:2D] = t_hat; catneg = [s_hat, -t_hat] (in_dtype of
 *              the GEMM), so that diff = cat * catneg^T = Gs - Gt in ONE batched NT GEMM with K = 2D;
 *              snorm [V][T] = max(||s||, eps) and a copy of s_hat alone (shat, GEMM dtype) for backward.
 *   sqsum:     loss[0] = scale * sum(diff^2)   (scale = 1/(V*T*T));  ws: [blocks] fp32, >= 1024 floats.
 *   normalize_bwd: dfeats[v][1+t] (+)= (dxh - xh (xh.dxh)) / norm  (dxh / eps when ||x|| <= eps);
 *              dfeats[v][0] untouched (CLS does not enter the Gram loss).
 * ------------------------------------------------------------------------------------------ */
int dinox_gram_normalize(const float* sfeats, const float* tfeats, void* cat, void* catneg, void* shat,
                         float* snorm, int V, int N, int D, int out_dtype, void* stream);
int dinox_sqsum(const float* x, int64_t n, float scale, float* loss, float* ws, void* stream);
int dinox_gram_normalize_bwd(const float* dxh, const void* shat, const float* snorm, const float* sfeats,
                             float* dfeats, int V, int N, int D, int shat_dtype, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * View pipeline for the 2.5D slice stacks -- replaces, after the PNG decode, PngDataset._load_hu01 and the
 * torchvision transform stack (scripts/phase5_big_run.py:493-497, 516-528, 549-555): stored u16 -> HU ->
 * window -> RandomResizedCrop (antialiased bicubic = torch's _upsample_bicubic2d_aa, align_corners = 0) ->
 * horizontal flip -> (x - mean) / std, one kernel, out = fp32 [V][3][S][S] (the batch PatchViT.forward takes).
 * The random draws stay on the host:  view_i[v] = {element offset of the (3,H,W) u16 stack in raw, H, W, top,
 * left, h, w, flip};  view_f[v] = {level - width/2, max(width, 1)}   (both tables in device memory).
 * max_crop = the largest h or w in the table (sizes the LDS footprint; a view that exceeds it is written as NaN).
 * Tested as stated (tests/test_resample_bounds_gpu.py): the tables sized from the true max_crop always suffice; when max_crop is
 * understated, a 16 x 16 output tile whose tap table or source footprint does not fit is written as NaN, whole -- nothing is read or
 * written out of range -- and every other tile is computed as usual.  More than 150 KiB of LDS
 * (dinox_slice_views_lds_bytes): DINOX_EUNSUPPORTED before any launch, out untouched.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_slice_views_lds_bytes(int S, int max_crop);
int dinox_slice_views(const void* raw_u16, const int64_t* view_i, const float* view_f, float* out, int V, int S, int max_crop,
                      void* stream);
/* The same pipeline writing the patch-embed operand directly: u[(v P + gy g + gx)][c p^2 + py p + px] (row stride ld >= 3 p^2,
 * g = S / patch, out_dtype DINOX_BF16 | DINOX_F32; columns 3 p^2 .. ld-1 are zeroed) -- bit for bit what dinox_patch_unfold(_ld)
 * makes of dinox_slice_views' output, without writing and re-reading the fp32 image batch (4 + 4 B per pixel). */
int dinox_slice_views_patches(const void* raw_u16, const int64_t* view_i, const float* view_f, void* u, int V, int S, int max_crop,
                              int patch, int ld, int out_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Inference-side preprocessing -- replaces the host code of zoo.encode (reference zoo/encode.py:34-72,129-157): source
 * element -> fp32 -> format -> window -> PIL Image.BILINEAR resize of a mode-F image to S x S -> (v - mean_c) / std_c,
 * one kernel, out = fp32 [n_images][3][S][S].
 *   format  HU_FLOAT: as is;  HU16_PNG: (u - 32768) * 0.1;  WINDOWED_FLOAT: as is and no window.
 *   window  clip(x, lo, hi), then (x - lo) / (hi - lo), a true fp32 division; lo and hi arrive as the doubles the reference
 *           computes (level -+ width / 2) and are rounded as NumPy rounds them against an fp32 array.
 *   resize  separable, horizontal first, fp32 intermediate; n -> S: scale = n / S, fs = max(scale, 1); output i has centre
 *           (i + .5) scale, taps [max(int(centre - fs + .5), 0), min(int(centre + fs + .5), n)), weight max(0, 1 - |(x - centre
 *           + .5) / fs|) renormalised to sum 1 (weights in double, sums in fp32).  n == S is the identity to the bit.
 * The unit of work is a plane job: jobs[j] = {element offset of the plane in src, H, W, row stride, pixel stride (both in
 * elements), number of destinations 1..3, three destinations image * 3 + channel (-1: unused)}, int64 [n_jobs][9] in device
 * memory.  The plane is filtered once and written to each destination with that channel's mean / std -- a replicated (H, W)
 * image is one job, plane z of a volume feeds the three 2.5D stacks it shows in.  The caller guarantees that every job stays
 * inside src; a destination outside [0, 3 n_images) is skipped.  src_dtype: DINOX_U16 | DINOX_I16 | DINOX_F32, one per launch.
 * max_side = the largest H or W in the table (sizes the LDS footprint; a plane that exceeds it is written as NaN).  More than
 * 150 KiB of LDS (dinox_encode_preprocess_lds_bytes): DINOX_EUNSUPPORTED before any launch.  n_jobs <= 65535.
 * Tested as stated (tests/test_resample_bounds_gpu.py): a 16 x 16 output tile whose tap table or footprint does not fit the tables
 * sized from max_side is written as NaN, whole, to every destination of its job; a destination index outside [0, 3 n_images) is
 * skipped and the job's other destinations are written; a job whose number of destinations is outside 1..3 is poisoned: NaN goes
 * to each of its three slots that names a destination inside the range, and to nothing else.
 * ------------------------------------------------------------------------------------------ */
#define DINOX_FMT_HU_FLOAT 0
#define DINOX_FMT_HU16_PNG 1
#define DINOX_FMT_WINDOWED_FLOAT 2
int64_t dinox_encode_preprocess_lds_bytes(int S, int max_side);
int dinox_encode_preprocess(const void* src, int src_dtype, const int64_t* jobs, int n_jobs, float* out, int n_images, int S,
                            int max_side, double lo, double hi, int format, void* stream);

/* ------------------------------------------------------------------------------------------
 * KoLeo regulariser -- replaces KoLeoLoss.forward (scripts/phase5_big_run.py:742-773), which the loop applies
 * to the student head output (:1764-1766): x^ = F.normalize(x); d_i = min_{j != i} ||x^_i - x^_j||;
 * loss = -mean_i log(d_i + eps).  fp32 throughout.  The all-pairs products G = X^_local X^_all^T go through
 * dinox_gemm (fp32); these entries are the pieces around it.  "local" rows are this rank's V_l rows, at
 * global positions row0 .. row0+V_l-1 of the V_g gathered rows (V_l = V_g, row0 = 0 on one GPU).
 *   normalize: xh = x / max(||x||, eps); norm[r] = ||x_r||; sq[r] = ||xh_r||^2.
 *   nn:        idx[i] = argmin_{j != row0+i} (sq_i + sq_j - 2 G[i][j]) (lowest j on ties; -1 if V_g = 1),
 *              dist[i] = ||xh_i - xh_idx|| measured on the rows themselves.
 *   bwd:       dx[r] = d(-gscale * sum_i log(dist_i + eps)) / dx_r over ALL V_g pairs (idx_all/dist_all are
 *              the gathered results of nn): the row's own pair plus every pair that chose r as neighbour,
 *              then back through the normalisation (norm_eps = the eps given to normalize).
 *              gscale = upstream gradient / V_l.  V_g <= 15359.
 * ------------------------------------------------------------------------------------------ */
int dinox_koleo_normalize(const float* x, float* xh, float* norm, float* sq, int64_t V, int D, float eps, void* stream);
int dinox_koleo_nn(const float* G, int64_t ldg, const float* sq_all, const float* xh_all, int row0, int V_l, int V_g, int D,
                   int* idx, float* dist, void* stream);
/* loss[0] = -mean_i log(dist[i] + eps) over the V local rows (fixed summation order). */
int dinox_koleo_loss(const float* dist, int V, float eps, float* loss, void* stream);
int dinox_koleo_bwd(const float* xh_all, const int* idx_all, const float* dist_all, const float* norm_loc, int row0, int V_l,
                    int V_g, int D, float gscale, float eps, float norm_eps, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * NT-Xent (SimCLR) loss head -- replaces SimCLRLoss.forward (scripts/phase5_big_run.py:776-813, used at :1728-1737) and its
 * backward: z^ = F.normalize(z) over the M = 2B rows [z1; z2] (dinox_koleo_normalize with eps = 1e-12); S = Z^ Z^T and
 * dZ^ = W Z^ through dinox_gemm (fp32); these entries are the pieces around them.  fp32 in both compute modes.
 * p(i) = (i + M/2) mod M is the row of i's positive; M even, >= 2.  Every sum has a fixed order (no atomics).
 *   rows:          lse[i] = logsumexp_{j != i} S[i][j] * inv_tau;  row_loss[i] = lse[i] - S[i][p(i)] * inv_tau;
 *                  loss[0] = (sum_i row_loss[i]) / M, added in index order.
 *   coeff:         W[i][j] = gscale * inv_tau / M * (exp(S_ij inv_tau - lse_i) + exp(S_ji inv_tau - lse_j) - [j = p(i)] - [i = p(j)]),
 *                  W[i][i] = 0, so that d(gscale * loss)/dZ^ = W Z^.  S_ij and S_ji are both read; W must not alias S.
 *   normalize_bwd: through xh = x / max(||x||, eps) with norm[r] = ||x_r||:  dx = (dxh - xh (xh . dxh)) / ||x||, and
 *                  dx = dxh / eps for rows with ||x|| < eps (torch's clamp_min backward).
 * ------------------------------------------------------------------------------------------ */
int dinox_ntxent_rows(const float* S, int64_t lds, int M, float inv_tau, float* lse, float* row_loss, float* loss, void* stream);
int dinox_ntxent_coeff(const float* S, int64_t lds, const float* lse, int M, float inv_tau, float gscale, float* W, int64_t ldw,
                       void* stream);
int dinox_normalize_bwd(const float* dxh, const float* xh, const float* norm, float* dx, int64_t V, int D, float eps, void* stream);
/* Rectangular forms for data parallelism: a rank holds Ml = 2 Bl local rows [z1_local; z2_local]; S [Ml][Mg] is their product with the
 * Mg = world * Ml gathered rows (all_gather_into_tensor order: rank r's block starts at row0 = r * Ml).  For local row i the excluded
 * column is dg(i) = row0 + i and the positive is p(i) = row0 + (i + Bl) mod Ml; world = 1, row0 = 0 are the square rules.
 *   rows_rect:  lse[i] = logsumexp_{j != dg(i)} S[i][j] * inv_tau;  row_loss[i] = lse[i] - S[i][p(i)] * inv_tau;
 *               loss_sum[0] = sum_i row_loss[i], added in index order and NOT divided (the caller adds the ranks' sums and divides by Mg).
 *   coeff_rect: W[i][j] = gscale * inv_tau / Ml * (exp(S_ij inv_tau - lse_local[i]) + exp(S_ij inv_tau - lse_all[j]) - 2 [j = p(i)]),
 *               W[i][dg(i)] = 0.  The second term is P_ji with S_ij standing in for S_ji (which another rank holds; the product is
 *               symmetric up to rounding) and lse_all [Mg] the gathered lse.  W Z^_all is Mg / Ml = world times the gradient of the
 *               global mean loss with respect to the local Z^: the factor the sum over ranks and AdamW's 1 / world take out again.
 * DINOX_EINVAL before any launch: Ml odd or < 2, Bl * 2 != Ml, Mg not a multiple of Ml, row0 not a multiple of Ml or outside
 * [0, Mg - Ml], lds < Mg, ldw < Mg, inv_tau <= 0, a null pointer. */
int dinox_ntxent_rows_rect(const float* S, int64_t lds, int Ml, int Mg, int row0, int Bl, float inv_tau, float* lse, float* row_loss,
                           float* loss_sum, void* stream);
int dinox_ntxent_coeff_rect(const float* S, int64_t lds, const float* lse_local, const float* lse_all, int Ml, int Mg, int row0, int Bl,
                            float inv_tau, float gscale, float* W, int64_t ldw, void* stream);

/* ------------------------------------------------------------------------------------------
 * MAE masked-token glue -- replaces MaeModel.random_masking / forward / patchify / forward_loss and the un-shuffle of
 * MaeDecoder.forward (scripts/phase5_big_run.py:816-1023) and their backward.  V samples of L = (H/patch)(W/patch) patches, of which
 * the Lk of lowest noise are kept.  ids_restore [V][L] int32 = rank of every patch; ids_keep [V][Lk] int32 = patch of every kept rank.
 * A patch is "removed" when its rank is outside [0, Lk).  Limits: 1 <= V <= 2^20, 2 <= L <= 4096, 1 <= Lk < L, 1 <= D <= 65536,
 * patch <= 32 for the loss entries; anything else, a null pointer or a dtype other than DINOX_F32 / DINOX_BF16 returns DINOX_EINVAL
 * before any launch.  Indices read from ids_* are range-checked on the device before use: an ids_restore entry outside [0, Lk) (negative
 * or too large) counts as removed and is never used as a row; an ids_keep entry is clamped into [0, L) (below 0 -> patch 0, L and above
 * -> patch L - 1).  Nothing outside the operands is read or written for any index value; the loss divisor stays V (L - Lk).
 * No float atomics; every sum has a fixed order.
 *   mask_ids:      ids_restore[v][p] = #{q : noise[v][q] < noise[v][p], or equal and q < p} (torch.argsort(stable=True) twice; -0 == +0,
 *                  NaN above everything); ids_keep[v][r] = p where the rank r < Lk.  One workgroup per sample.
 *   gather_unfold: u[(v Lk + r)][c p p + py p + px] = x[v][c][gy p + py][gx p + px] for patch ids_keep[v][r] = gy (W/p) + gx, rows of
 *                  ld >= 3 p^2 elements with a zero tail: rows v L + ids_keep[v][r] of dinox_patch_unfold / _ld, bit for bit.
 *   tokens_fwd:    tokens [V][1 + Lk][D] fp32: [v][0] = cls + pos[0];  [v][1 + r] = patches[v][r] + pos[1 + ids_keep[v][r]].
 *   tokens_bwd:    dpatches[v][r] = dtokens[v][1 + r] (operand dtype);  dpos[0] = dcls = sum_v dtokens[v][0];
 *                  dpos[1 + p] = sum_{v : ids_restore[v][p] < Lk} dtokens[v][1 + ids_restore[v][p]], ascending v (dpos is [1 + L][D]).
 *   unshuffle_fwd: xd [V][1 + L][D] fp32: [v][0] = e[v][0] + dec_pos[0];  [v][1 + p] = (kept ? e[v][1 + ids_restore[v][p]] : mask_token)
 *                  + dec_pos[1 + p];  e is [V][1 + Lk][D] in e_dtype.
 *   unshuffle_bwd: de[v][0] = g[v][0], de[v][1 + r] = g[v][1 + ids_keep[v][r]] (de_dtype);  dmask_token = sum of g over the removed
 *                  (v, p): per sample in ascending p into ws [V][D] fp32, then over ascending v.  dec_pos gets no gradient.
 *   loss_fwd:      pred [V][lead + L][3 p^2] (lead = 1: the CLS row is still in front; 0: it was dropped), target pixel
 *                  x[v][c][gy p + py][gx p + px] at column (py p + px) 3 + c, read from the image.
 *                  loss[0] = sum_{removed (v,l)} mean_j (pred - target)^2 / (V (L - Lk));  ws: V L floats (the per-patch means).
 *   loss_bwd:      dpred (same layout, dpred_dtype) = gscale 2 (pred - target) / (3 p^2 V (L - Lk)) on removed patches, exactly 0 on kept
 *                  ones and on the lead rows.  dpred must not alias pred.
 * ------------------------------------------------------------------------------------------ */
int dinox_mae_mask_ids(const float* noise, int* ids_restore, int* ids_keep, int V, int L, int Lk, void* stream);
int dinox_mae_gather_unfold(const float* x, const int* ids_keep, void* u, int V, int H, int W, int patch, int Lk, int ld, int out_dtype,
                            void* stream);
int dinox_mae_tokens_fwd(const void* patches, const float* cls, const float* pos, const int* ids_keep, float* tokens, int V, int L, int Lk,
                         int D, int patches_dtype, void* stream);
int dinox_mae_tokens_bwd(const float* dtokens, const int* ids_restore, void* dpatches, float* dcls, float* dpos, int V, int L, int Lk, int D,
                         int patches_dtype, void* stream);
int dinox_mae_unshuffle_fwd(const void* e, const float* mask_token, const float* dec_pos, const int* ids_restore, float* xd, int V, int L,
                            int Lk, int D, int e_dtype, void* stream);
int dinox_mae_unshuffle_bwd(const float* g, const int* ids_keep, const int* ids_restore, void* de, float* dmask_token, float* ws, int V,
                            int L, int Lk, int D, int de_dtype, void* stream);
int dinox_mae_loss_fwd(const void* pred, const float* x, const int* ids_restore, float* loss, float* ws, int V, int H, int W, int patch,
                       int Lk, int lead, int pred_dtype, void* stream);
int dinox_mae_loss_bwd(const void* pred, const float* x, const int* ids_restore, void* dpred, float gscale, int V, int H, int W, int patch,
                       int Lk, int lead, int pred_dtype, int dpred_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * iBOT masked-patch objective (extension; iBOT / DINOv2, not in the reference).  idx [M] int32 ON THE DEVICE: distinct flat patch
 * positions v P + i of the [rows = V P][D] patch-product output.  An entry outside [0, rows) (or [0, src_rows) / [0, dst_rows)) is
 * skipped: nothing is read or written for it.  fp32 math, fixed summation order, no atomics, no allocation, no synchronisation.
 *   put_mask:         patches[idx[m]][:] = mask_token [D] fp32, rounded to `dtype`, in place.
 *   put_mask_bwd:     dmask_token[d] = sum_m dpatches[idx[m]][d], ascending m within chunks of 64 rows, then the chunks in order
 *                     (ws: ceil(M / 64) * D floats); then those rows of dpatches are set to exactly 0.  M <= 65535 * 64.
 *   gather_rows:      dst[dst_row0 + m][:] = src[row[m]][:]   (src fp32 [src_rows][D]; dst in dst_dtype): dinox_take_rows by index.
 *   scatter_add_rows: dst[row[m]][:] += src[src_row0 + m][:]  (dst fp32 [dst_rows][D]); the rows must be distinct.
 *   ibot_ce:          s, t [M][K] fp32, center [K], w [M]:  p_t[m] = softmax((t[m] - center) / teacher_temp),
 *                     row_loss[m] = -sum_k p_t[m][k] log_softmax(s[m] / student_temp)[k],   loss[0] = scale * sum_m w[m] row_loss[m]
 *                     (one workgroup, index order),   ds[m] = grad_scale * scale * w[m] * (softmax(s[m] / student_temp) - p_t[m]) /
 *                     student_temp, or ds NULL.  ds must not overlap s or t.  Log-sum-exp form: finite inputs give finite outputs.
 *                     K % 4 == 0, K <= 8192 and 16-byte aligned s, t, center, ds: every row is loaded once and held in registers
 *                     (each matrix crosses the bus once); anything else takes a scalar kernel that re-reads the row.
 *   ibot_center_ema:  center[k] = center[k] momentum + (sum_count[k] / sum_count[K]) (1 - momentum): the patch centre from the column
 *                     sums of the masked teacher rows and their number (sum_count [K + 1] fp32, possibly added up over ranks); a number
 *                     below 1 leaves the centre untouched.
 * DINOX_EINVAL before any launch: a null pointer (ds excepted), M < 1, K < 1, D < 1, rows < 1, a temperature <= 0, a dtype other than
 * DINOX_F32 / DINOX_BF16.
 * ------------------------------------------------------------------------------------------ */
int dinox_ibot_put_mask(void* patches, const float* mask_token, const int* idx, int M, int64_t rows, int D, int dtype, void* stream);
int dinox_ibot_put_mask_bwd(void* dpatches, const int* idx, float* dmask_token, float* ws, int M, int64_t rows, int D, int dtype,
                            void* stream);
int dinox_gather_rows(const float* src, const int* row, void* dst, int64_t M, int64_t src_rows, int D, int64_t dst_row0, int dst_dtype,
                      void* stream);
int dinox_scatter_add_rows(const void* src, const int* row, float* dst, int64_t M, int64_t dst_rows, int D, int64_t src_row0, int src_dtype,
                           void* stream);
int dinox_ibot_ce(const float* s, const float* t, const float* center, const float* w, float student_temp, float teacher_temp, float scale,
                  float grad_scale, float* loss, float* ds, float* row_loss, int M, int K, void* stream);
int dinox_ibot_center_ema(float* center, const float* sum_count, float momentum, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention rows -- the softmax rows of a few query tokens (CLS, the registers) over all keys, per head: the attention map the
 * reference's roadmap asks for and its fused SDPA cannot return (scripts/phase5_monitor.py draws a patch-norm proxy instead).
 *   qkv        [B, N, 3, heads, d] packed as dinox_attention_fwd takes it, dtype DINOX_F32 or DINOX_BF16; V is never read
 *   query_idx  [Q] int32 ON THE DEVICE, each in [0, N); an entry outside turns its row and its lse into NaN (nothing is read for it)
 *   probs      [B, heads, Q, N] fp32 = softmax_j(q_i . k_j / sqrt(d)); also the kernel's score buffer, so it must not alias qkv
 *   lse        [B, heads, Q] fp32 log-sum-exp of the scaled scores, or NULL
 * fp32 scores (bf16 products are exact), fp32 maximum, sum and probabilities; fixed reduction order, no atomics: bit-reproducible.
 * One workgroup per (image, head).  1 <= Q <= 8, 1 <= d <= 256, B, N, heads >= 1 (dinox_attention_rows_ok: host only, 1 inside);
 * anything else returns DINOX_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int dinox_attention_rows_ok(int B, int N, int heads, int d, int Q);
int dinox_attention_rows(const void* qkv, const int* query_idx, float* probs, float* lse, int B, int N, int heads, int d, int Q, int dtype,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * Attention rollout step -- one factor of the CLS row of attention rollout (Abnar & Zuidema 2020), with no N x N matrix stored:
 *   w_out[b][j] = residual w_in[b][j] + (1 - residual) / heads * sum_h sum_i w_in[b][i] * softmax_j(q_i . k_j / sqrt(d))
 * Chained from the last block down, starting from the one-hot vector of a query token, it gives that token's row of
 * Ahat_L ... Ahat_1, Ahat_l = residual I + (1 - residual) mean_h P_l^h.
 *   qkv        [B, N, 3, heads, d] packed as dinox_attention_fwd takes it, dtype DINOX_F32 or DINOX_BF16; V is never read
 *   w_in       [B, N] fp32;  w_out [B, N] fp32, must not overlap w_in
 *   ws         dinox_attention_rollout_step_ws_bytes(B, N, heads) bytes (= B heads N floats: the per-head partial sums)
 *   residual   in [0, 1]
 * fp32 scores (bf16 products are exact), fp32 maximum, sum and probabilities, as dinox_attention_rows; the column sum adds the query
 * rows in index order, the heads in index order; no atomics: bit-reproducible.  Query rows go by in chunks of 8; a chunk whose 8
 * weights are all exactly 0 is skipped (it would add exactly 0; a non-finite q in such a row is therefore not seen).
 * Two launches: one workgroup per (image, head), then one thread per (image, key).
 * Limits (dinox_attention_rollout_step_ok: host only, 1 inside): B, heads >= 1, 1 <= N <= 4096 (the 8 x N score rows of a chunk
 * sit in LDS), 1 <= d <= 256; anything else, a residual outside [0, 1], a null pointer or overlapping w returns DINOX_EINVAL before
 * any launch.  dinox_attention_rollout_step_ws_bytes returns 0 for every B, N, heads the call refuses.
 * ------------------------------------------------------------------------------------------ */
int dinox_attention_rollout_step_ok(int B, int N, int heads, int d);
size_t dinox_attention_rollout_step_ws_bytes(int B, int N, int heads);
int dinox_attention_rollout_step(const void* qkv, const float* w_in, float* w_out, void* ws, int B, int N, int heads, int d, float residual,
                                 int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser tail -- replaces the per-parameter grad-norm loop (scripts/phase5_big_run.py:1784-1789),
 * torch.optim.AdamW.step (:1794; betas .9/.999, eps 1e-8, decoupled decay on EVERY parameter) and the
 * per-parameter EMA teacher update (:1799-1802) with ONE pass over flat fp32 arenas of n elements.
 *   g is multiplied by grad_scale first (1/world_size after a sum all-reduce);
 *   gnorm_sq[0] = sum((grad_scale*g)^2)  (fp32; ws: >= 4096 floats);  teacher may be NULL (no EMA).
 *   step_t = 1-based optimiser step for the bias corrections.
 * cast: bf16 copies of weights for the MFMA path (and [C][R] transposed copies for dX products).
 * ------------------------------------------------------------------------------------------ */
int dinox_adamw_ema(float* p, const float* g, float* m, float* v, float* teacher, int64_t n, float lr,
                    float weight_decay, float beta1, float beta2, float eps, int step_t, float ema,
                    float grad_scale, float* gnorm_sq, float* ws, void* stream);
/* The same pass with its per-step scalars in DEVICE memory -- hyper[3] = {lr, 1/(1-beta1^t), 1/sqrt(1-beta2^t)} -- so that the
 * launch can sit in a captured hipGraph and be replayed with a new learning rate / step count (the host writes hyper before
 * each replay).  New in this engine (the reference has no graph capture); same arithmetic as dinox_adamw_ema. */
int dinox_adamw_ema_dev(float* p, const float* g, float* m, float* v, float* teacher, int64_t n, const float* hyper,
                        float weight_decay, float beta1, float beta2, float eps, float ema, float grad_scale,
                        float* gnorm_sq, float* ws, void* stream);
int dinox_sumsq(const float* x, int64_t n, float* out, float* ws, void* stream);
int dinox_cast_bf16(const float* src, void* dst, int64_t n, void* stream);
int dinox_cast_transpose_bf16(const float* src, void* dst, int R, int C, void* stream);
/* All matrices of a parameter arena in one launch: table (device, int64 [n_mats][4]) holds per matrix {element offset (the same
 * in src_base and dst_base), R, C, index of its first 32x32 tile}; total_tiles = sum of ceil(R/32)*ceil(C/32). */
int dinox_cast_transpose_bf16_multi(const float* src_base, void* dst_base, const int64_t* table, int n_mats,
                                    int64_t total_tiles, void* stream);
/* ------------------------------------------------------------------------------------------
 * Glue between the big kernels, so that no framework elementwise kernel runs inside a training step.
 *   take_rows: dst[dst_row0 + v][0..D) = src[v * src_stride + 0..D)   (fp32 -> dst_dtype).  With src = features + 0 and
 *              src_stride = N*D this is `feats[:, 0]` (the CLS row handed to the DINO head, zoo/arch.py:260-261).
 *   put_rows:  dst[v * dst_stride + 0..D) (+)= src[src_row0 + v][0..D)   (src_dtype -> fp32): the head's input gradient written
 *              into row 0 of the feature gradient (the reference's slice backward: zero fill + copy + full-size add).
 *   axpy:      y += alpha * x (fp32).     lincomb3: out[0] = a[0] + wb*b[0] + wc*c[0] (b, c may be NULL): the total loss
 *              (scripts/phase5_big_run.py:1755-1766).     zero: asynchronous zero fill.
 * ------------------------------------------------------------------------------------------ */
int dinox_take_rows(const float* src, void* dst, int64_t V, int64_t src_stride, int D, int64_t dst_row0, int dst_dtype,
                    void* stream);
int dinox_put_rows(const void* src, float* dst, int64_t V, int64_t dst_stride, int D, int64_t src_row0, int src_dtype,
                   int accumulate, void* stream);
int dinox_axpy(float* y, const float* x, float alpha, int64_t n, void* stream);
int dinox_lincomb3(const float* a, const float* b, const float* c, float wb, float wc, float* out, void* stream);
int dinox_zero(void* p, int64_t bytes, void* stream);
/* Elementwise helpers used by the host-side modules: y = gelu_erf(x) / dx = dy * gelu_erf'(x) (fp32). */
int dinox_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int dinox_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------
 * One pre-norm transformer block per call (bf16 throughput mode) -- the launch SEQUENCE of zoo/arch.py:94-97 with Attention :43-54 and
 * Mlp :75-76 inlined, enqueued by the library instead of by ~13 (forward) / ~15 (backward) calls from the host language:
 *     x1 = x0 + proj(attention(qkv(norm1(x0))));   x2 = x1 + fc2(gelu(fc1(norm2(x1))))
 * Same kernels, same order, same results as the entries above called one by one (LayerNorm, dinox_gemm with its fused epilogues,
 * dinox_attention_*, dinox_linear_residual_ln); still no allocation, no synchronisation, hipGraph-capturable, re-entrant: every tensor,
 * the saved activations of the backward pass and all workspaces are the caller's.  What it buys is host time: one foreign call per
 * block instead of one per launch (Python: 24 ms of enqueue per ViT-S bs-256 step before), under data parallelism and
 * gradient accumulation too.  All activations are row-major [V*N, .]; bf16 tensors are operands of the next product, fp32 ones the
 * residual stream, the statistics and the gradients.
 * forward:  xn1_in (+ mean1_in, rstd1_in) non-NULL = norm1(x0) was already produced by the previous block's epilogue; then xn1 /
 *           mean1 / rstd1 are not written.  fuse_proj_ln / fuse_fc2_ln: run the product and the LayerNorm behind it as ONE launch
 *           (dinox_linear_residual_ln; needs dinox_linear_residual_ln_ok).  next_g non-NULL: also return yn = LayerNorm(x2; next_g,
 *           next_b, next_eps) in next_dtype with its statistics (the next block's norm1, or the model's final norm).
 *           pre non-NULL (training): fc1 also writes gelu'(pre-activation) there (the DINOX_EPI_AUXGRAD side tensor).
 * backward: g = d loss / d x2 (fp32), g_lowp = its bf16 copy (NULL: cast here into g_lowp_buf).  Weight operands are the TRANSPOSED
 *           bf16 images W^T [in][out] (dX = dY . W as an NT product).  Parameter gradients are ACCUMULATED into dwqkv .. dn2b (slices
 *           of a gradient arena).  Scratch: dpre [M,H], dxn2 / d_o / dxn1 [M,D], dqkv [M,3D] bf16; g1 [M,D] fp32 and g1_lowp bf16.
 *           Outputs: g0 = d loss / d x0 written IN PLACE of g1 (same buffer), g0_lowp its bf16 copy.
 *           attn_ws: dinox_attention_bwd_ws_bytes; ln_ws: dinox_layernorm_bwd_ws_bytes(M, D) (used twice, in stream order);
 *           tn_ws / tn_ws_bytes: workspace of the deterministic dW products (>= the largest dinox_gemm_ws_bytes of the four).
 * plan:     dinox_block_forward / _backward do what their flags say; WHICH launches to fuse is decided in one place, dinox_block_plan
 *           (measured rules per shape; their A/B environment switches, read at every call, are listed in csrc/knobs.h).
 *           Ask it once per block forward, pass fuse_proj_ln / fuse_fc2_ln on, leave qkv NULL when qkv_fused, and hand
 *           fuse_ln_bwd to the backward of the same block.  Host logic only: no launch, nothing dereferenced but `out`.
 *           dtype = compute mode (DINOX_F32, the parity mode, fuses nothing: an all-zero plan); train != 0 = the pass keeps tensors
 *           for a backward; next_dtype = dtype of the LayerNorm that follows the block (next_g), or -1 when there is none.
 * ------------------------------------------------------------------------------------------ */
typedef struct dinox_block_plan_t {
  int32_t qkv_fused;      /* no-grad pass: qkv projection + attention as one launch (dinox_qkv_attention_fwd), no qkv tensor */
  int32_t fuse_proj_ln;   /* proj + residual + norm2 as dinox_linear_residual_ln */
  int32_t fuse_fc2_ln;    /* fc2 + residual + the LayerNorm that follows the block, likewise (0 when next_dtype < 0) */
  int32_t fuse_ln_bwd;    /* both dX products into the LayerNorms as dinox_linear_ln_bwd */
} dinox_block_plan_t;
int dinox_block_plan(int64_t V, int64_t N, int D, int H, int heads, int dtype, int train, int next_dtype, dinox_block_plan_t* out);

typedef struct dinox_block_fwd_args {
  int64_t V, N;                        /* views, tokens per view: M = V * N rows */
  int32_t D, H, heads;                 /* width, MLP hidden width, attention heads */
  int32_t train;                       /* != 0: `pre` receives the GELU' side tensor */
  int32_t fuse_proj_ln, fuse_fc2_ln;
  float eps;                           /* of norm1 / norm2 */
  const float* x0;
  const void* xn1_in; const float* mean1_in; const float* rstd1_in;
  void* xn1; float* mean1; float* rstd1;
  void* qkv; void* o; float* lse;
  float* x1; void* xn2; float* mean2; float* rstd2;
  void* act; void* pre;
  float* x2;
  const float* next_g; const float* next_b; float next_eps; int32_t next_dtype;
  void* yn; float* meann; float* rstdn;
  const float *n1w, *n1b, *n2w, *n2b;
  const void *wqkv, *wproj, *w1, *w2;  /* bf16 [3D,D], [D,D], [H,D], [D,H] */
  const float *bqkv, *bproj, *b1, *b2; /* fp32 or NULL */
} dinox_block_fwd_args;

typedef struct dinox_block_bwd_args {
  int64_t V, N;
  int32_t D, H, heads;
  int32_t fuse_ln_bwd;                          /* != 0: the two dX products into the LayerNorms run dinox_linear_ln_bwd */
  const float* g; const void* g_lowp; void* g_lowp_buf;
  /* saved by the forward */
  const float* x0; const float* x1; const void* xn1; const void* xn2; const void* qkv; const void* o; const float* lse;
  const void* pre; const void* act; const float *mean1, *rstd1, *mean2, *rstd2;
  const float *n1w, *n2w;
  const void *wqkv_t, *wproj_t, *w1_t, *w2_t;   /* bf16 W^T: [D,3D], [D,D], [D,H], [H,D] */
  /* gradient arena slices (accumulated into); bias gradients may be NULL */
  float *dwqkv, *dbqkv, *dwproj, *dbproj, *dw1, *db1, *dw2, *db2, *dn1w, *dn1b, *dn2w, *dn2b;
  /* scratch and outputs */
  void* dpre; void* dxn2; void* d_o; void* dqkv; void* dxn1;
  float* g1; void* g1_lowp; void* g0_lowp;
  void* attn_ws; void* ln_ws; void* tn_ws; int64_t tn_ws_bytes;
} dinox_block_bwd_args;

int dinox_block_forward(const dinox_block_fwd_args* args, void* stream);
int dinox_block_backward(const dinox_block_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * View-retrieval rank -- replaces the host block of scripts/phase5_view_retrieval_eval.py:214-227 (S = Q K^T as an N x N numpy array,
 * np.argmax / np.argpartition over its rows).  No Nq x Nk array exists: the similarity tiles live in the accumulators of the exact-fp32
 * MFMA and leave them as counts.  q [Nq][D] (ldq >= D) and k [Nk][D] (ldk >= D) are fp32 rows, used as given (pass unit rows:
 * dinox_koleo_normalize with eps = 1e-12 is F.normalize); target[i] is the index of query i's positive key (NULL: target[i] = i,
 * needs Nq == Nk).  With s(i,j) = sum_d q[i][d] k[j][d], fp32, ascending d:
 *   pos_val[i]  = s(i, target[i]), bitwise the value the sweep computes for that column;
 *   rank[i]     = #{j : s(i,j) > pos_val[i]} + #{j < target[i] : s(i,j) == pos_val[i]}  -- the positive's place in a stable descending
 *                 sort; rank == 0 is exactly np.argmax(S[i]) == target[i], rank < k is "among the k nearest";
 *   best_val[i] = max_j s(i,j), best_idx[i] = its lowest index.
 * ws: dinox_retrieval_ws_bytes(Nq, Nk, D) bytes (12 bytes per query and key split, a pure function of the three sizes, 0 for sizes the call refuses; contents need not be
 * initialised).  Any Nq, Nk, D >= 1 (Nq, Nk <= 2^31 - 129).
 * Caller's contract: 0 <= target[i] < Nk.  An index outside that range is CLAMPED into it (it never becomes an address), so the outputs
 * of that query then describe key 0 or key Nk - 1; dinox.ops.retrieval_rank checks the range before the call.
 * Non-finite scores: every comparison with a NaN is false, so a query row of NaNs gets rank 0, best_idx = 0x7fffffff, best_val = -inf and a
 * NaN pos_val; test pos_val (dinox.retrieval.view_retrieval does) before reading a score from such rows.
 * Three launches on the stream, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_retrieval_ws_bytes(int64_t Nq, int64_t Nk, int64_t D);
int dinox_retrieval_rank(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* target, int64_t Nq, int64_t Nk, int64_t D,
                         int32_t* rank, int32_t* best_idx, float* best_val, float* pos_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Windowed view-retrieval rank -- the per-dataset view retrieval of scripts/evaluate_panorgan.py (metric 1: one Q K^T per dataset) as ONE
 * call over the concatenated rows.  The semantics of dinox_retrieval_rank with every "over j" restricted to the window of query i,
 * key_lo[i] <= j < key_hi[i]:
 *   pos_val[i]  = s(i, target[i]);
 *   rank[i]     = #{j in window : s(i,j) > pos_val[i]} + #{j in window, j < target[i] : s(i,j) == pos_val[i]};
 *   best_val[i] = the maximum over the window, best_idx[i] = its lowest index, a GLOBAL key index.
 * target == NULL means target[i] = i and needs Nq == Nk.  s(i,j) is BITWISE the score dinox_retrieval_rank computes for the same operands
 * (same tile loop, key tiles at multiples of 128 of the global key index): a window of [0, Nk) for every query reproduces that entry bit
 * for bit, and a window equal to a row range reproduces the call on that range (best_idx shifted by the range's start).
 * Work: a strip of 128 queries sweeps only the key tiles one of its windows touches, so with rows sorted by group the cost is
 * sum n_g^2 scores, not Nq Nk.  Windows may be arbitrary and unsorted (the cost is then the tiles each strip's windows touch).
 * ws: dinox_retrieval_rank_windowed_ws_bytes(Nq, Nk, D) bytes (12 bytes per query and key split, a pure function of the sizes, 0 for sizes the call refuses; contents
 * need not be initialised).  Any Nq, Nk, D >= 1 (Nq, Nk <= 2^31 - 129), ldq, ldk >= D.
 * Bad input never becomes an address or a loop bound: key_lo[i] and key_hi[i] are CLAMPED into [0, Nk] and target[i] into [0, Nk) as
 * in dinox_retrieval_rank.  An empty window (lo >= hi after clamping) gives rank 0, best_idx = 0x7fffffff, best_val = -inf; pos_val is
 * still written.  A target outside its window is allowed: rank is the place the target would take among the window's keys.
 * Non-finite scores behave as documented for dinox_retrieval_rank (a NaN query row: rank 0, best_idx = 0x7fffffff, best_val = -inf, NaN
 * pos_val; test pos_val).  Three launches on the stream, plain stores, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_retrieval_rank_windowed_ws_bytes(int64_t Nq, int64_t Nk, int64_t D);
int dinox_retrieval_rank_windowed(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* target, const int32_t* key_lo,
                                  const int32_t* key_hi, int64_t Nq, int64_t Nk, int64_t D, int32_t* rank, int32_t* best_idx, float* best_val,
                                  float* pos_val, void* ws, void* stream);

/* Paired row dot products: out[i] = sum_d a[i][d] b[i][d] for fp32 rows a [N][D] (lda >= D), b [N][D] (ldb >= D) -- BITWISE pos_val[i] of
 * dinox_retrieval_rank(q = a, k = b, target = NULL): the first of its launches on its own (same operand roles, same ascending-d fp32 chain
 * on the exact-fp32 MFMA), no workspace, no sweep.  The cosine distance of the spacing counterfactual (metric 3) is 1 - out[i] of unit rows. */
int dinox_row_dots(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t N, int64_t D, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * K nearest keys -- replaces the host block of scripts/evaluate_panorgan.py:526-529 (S = E E^T as an N x N numpy array, fill_diagonal(-inf),
 * np.argpartition over its rows) and feeds the weighted k-NN probe.  Same operands, same score as dinox_retrieval_rank (exact-fp32 MFMA, one
 * d-ordered fp32 fma chain per score; the two entries share the tile loop): for equal operands out_val[i][0], out_idx[i][0] are BITWISE
 * best_val[i], best_idx[i] of dinox_retrieval_rank.
 *   row i of out_idx / out_val [Nq][K] = the first K keys in the order (score descending, index ascending) -- a total order, the result is
 *   unique -- with key exclude[i] left out (exclude = NULL or exclude[i] = -1: nothing left out; exclude[i] = i is the reference's
 *   fill_diagonal(-inf)).  exclude[i] is only ever COMPARED with key indices: a value outside [0, Nk) leaves nothing out and never becomes an
 *   address.  1 <= K <= 32, anything else returns DINOX_EINVAL.  Fewer than K eligible keys: the remaining slots hold index -1 and value -inf.
 * ws: dinox_knn_ws_bytes(Nq, Nk, D, K) bytes (8 K bytes per query and key split; the splits are a pure function of Nq and Nk, never more
 * than dinox_retrieval_rank uses; 0 for every Nq, Nk, D, K the call refuses; contents need not be initialised).  Any Nq, Nk, D >= 1 (Nq, Nk <= 2^31 - 129), ldq, ldk >= D.
 * Non-finite scores: a NaN score compares false with everything and never enters a row, so a query row of NaNs returns K times (-1, -inf) and
 * a NaN key is never a neighbour; no ordering promise is made for rows that meet NaNs, but no address depends on a score and no loop on a
 * comparison: such rows neither fault nor hang.
 * Two launches on the stream, plain stores, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_knn_ws_bytes(int64_t Nq, int64_t Nk, int64_t D, int K);
int dinox_knn_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* exclude, int64_t Nq, int64_t Nk, int64_t D, int K,
                   int32_t* out_idx, float* out_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * One step of dense label propagation (Caron et al. 2021, the video-segmentation protocol of DINO; here the sequence is the z axis of a
 * series): for every patch of the target slice the K best-matching patches of F context slots inside a spatial window, then a
 * softmax-weighted vote over their soft labels.  No [N][F N] affinity matrix is ever held.
 *   q   fp32 [N][D], row stride ldq: the patch features of the target slice, N = g g, patch p = y g + x
 *   k   fp32 [F N][D], row stride ldk: the patch features of the F context slots, key j = f N + y' g + x'
 *   seg fp32 [F N][C], contiguous: the soft labels of the context patches (a row may be all zero)
 * Candidates of p = (y, x): the keys (f, y', x') with |y' - y| <= radius and |x' - x| <= radius, the window clipped at the grid border;
 * radius < 0 or radius >= g - 1: the whole grid.
 * Score: s(p, j) = sum_d q[p][d] k[j][d], the tile loop of dinox_knn_topk (exact-fp32 MFMA, one d-ordered fma chain): BITWISE its score.
 * Selection: row p of out_idx / out_val [N][K] = the first K candidates in the order (score descending, key index ascending), the total
 * order of dinox_knn_topk: with a whole-grid radius the two rows equal dinox_knn_topk(q, k, exclude = NULL) bitwise.  Fewer than K
 * candidates: the remaining slots hold (-1, -inf).  A NaN score never enters: a NaN query row returns K times (-1, -inf), a NaN key is
 * never chosen; rows that meet NaNs neither fault nor hang (no address depends on a score, no loop on a comparison).
 * Vote over the filled slots i = 1..n of row p (a prefix):  w_i = exp((s_i - s_1) inv_temperature),
 *   out[p][c] = sum_i w_i seg[j_i][c] / sum_i w_i,   fp32 [N][C], NOT renormalised over c; a row with no filled slot is all zero.
 * The exponent argument is rounded to fp32 once, exp is within 1 ulp, the numerator is one fp32 fma chain over i ascending, the
 * denominator is summed over i ascending in fp32 with compensation (one rounding), then one division.
 * Tile skipping: a tile of 128 consecutive keys is neither loaded nor multiplied when none of its keys lies in a grid row within radius
 * of a grid row of the 128 consecutive patches of the query strip; the window proper is tested per (patch, key) at selection.
 * 1 <= K <= 32, 2 <= C <= 64, g, F, D >= 1, F g g <= 2^31 - 129, ldq, ldk >= D, inv_temperature finite and > 0; anything else, or a null
 * pointer, returns DINOX_EINVAL before any launch.
 * ws: dinox_labelprop_ws_bytes(g, F, D, C, K) bytes (8 K bytes per patch and key split; a pure function of g and F; 0 for every argument
 * set the call refuses; contents need not be initialised).  Two launches on the stream, plain stores, a fixed merge order of the key
 * splits, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_labelprop_ws_bytes(int g, int F, int D, int C, int K);
int dinox_labelprop(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* seg, int g, int F, int D, int C, int K, int radius,
                    float inv_temperature, float* out, int32_t* out_idx, float* out_val, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * Second moments of the columns of x [N][D] fp32 (ldx >= D) -- replaces the host NumPy / scikit-learn passes of the reference's ridge and
 * embedding-statistics metrics (scripts/evaluate_panorgan.py:569-697).  With z_i = x_i - shift (ONE fp32 subtraction per element; shift
 * NULL: z = x):   gram[a][b] = sum_i z_ia z_ib  (double [D][D], symmetric to the bit),   colsum[a] = sum_i z_ia  (double [D]).
 * Append a target column to x to read X^T y and y^T y from the same pass.  1 <= D <= 1024, N >= 1; anything else returns DINOX_EINVAL.
 * Exact-fp32 MFMA products summed in fp32 over a split of the rows (at most ceil(N / splits) + 15 terms, in row order), the splits then
 * summed in ascending order in double: |error of gram[a][b]| <= N 2^-24 sum_i |z_ia z_ib|.  Rows past N and columns past D enter as
 * exact zeros.  Non-finite inputs propagate into the sums they belong to and neither fault nor hang.
 * ws: dinox_gram_ws_bytes(N, D) bytes (a pure function of the two sizes; 0 for sizes the call refuses; contents need not be
 * initialised).  Two launches on the stream, plain stores, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_gram_ws_bytes(int64_t N, int64_t D);
int dinox_gram_f32(const float* x, int64_t ldx, int64_t N, int64_t D, const float* shift, double* gram, double* colsum, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * One evaluation of a multinomial logistic (softmax) probe -- the inner step of the reference's dataset-discrimination metric
 * (scripts/evaluate_panorgan.py:375-379, scikit-learn's LogisticRegression on the host).  x [N][D] fp32 rows (ldx >= D), label int32 [N],
 * theta fp32 [C][D + 1] with the intercept in the last column:
 *   z_ic = theta_c[:D] . x_i + theta_c[D],   p_i = softmax(z_i)  (log-sum-exp form: no overflow at any finite logit),
 *   loss[0]  = sum_i (logsumexp(z_i) - z_i,label_i)                       double, or NULL
 *   grad     = sum_i (p_ic - [label_i == c]) [x_i, 1]                     double [C][D + 1], or NULL
 *   prob     = p                                                          fp32 [N][C], or NULL
 * loss == NULL && grad == NULL is the predict form; the probabilities are bitwise the same in both forms.  2 <= C <= 32, 1 <= D <= 1024,
 * N >= 1, at least one output; anything else returns DINOX_EINVAL.  A row whose label is outside [0, C) contributes nothing to loss and
 * grad (its prob row is still written); a label is only ever COMPARED with class numbers and never becomes an address.
 * Logits and R^T X on the exact-fp32 MFMA; the rows are read once.  Per-workgroup fp32 partial gradients (row order) and double partial
 * losses are added in ascending workgroup order in double.  Non-finite inputs propagate and neither fault nor hang.
 * ws: dinox_softmax_probe_ws_bytes(N, D, C) bytes, 8-byte aligned (a pure function of the sizes; 0 for sizes the call refuses; contents
 * need not be initialised).  One launch (predict form) or two on the stream, plain stores, no atomics: results are bit-reproducible.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_softmax_probe_ws_bytes(int64_t N, int64_t D, int C);
int dinox_softmax_probe(const float* x, int64_t ldx, const int32_t* label, int64_t N, int64_t D, int C, const float* theta, double* loss,
                        double* grad, float* prob, void* ws, void* stream);

/* ------------------------------------------------------------------------------------------
 * LoRA: the low-rank side of a wrapped linear layer (kernels: csrc/lora.hip; autograd node: dinox.ops.LoraLinearFn).  One layer is
 *   y = x W^T + b + s (xl A^T) B^T (+ residual),   x [M][K], W [N][K], A [r][K], B [N][r], s = alpha / r, xl = x or dropout(x).
 * The base product stays dinox_gemm; the low-rank term reaches it as its fp32 RESIDUAL input, so it is never folded into a bf16 weight.
 * A, B, u = xl A^T, v = dy B and every sum are fp32; `dtype` is the dtype of the activation operand (DINOX_F32 or DINOX_BF16).
 * Every entry checks its arguments on the host (DINOX_EINVAL and a message before any launch), allocates nothing, does not synchronise,
 * uses plain stores only and a fixed summation order: equal inputs give equal bits.  1 <= r <= 64; M, K, N >= 1; M <= 2^31 - 1;
 * K, N <= 2^20; rows are dense (row stride = row length).
 *
 * dinox_lora_down:  u[M][r] (fp32) = x[M][K] . S, one ascending-k chain per lane and a fixed wave tree.  small_layout 0: S is stored [r][K]
 *   (u = xl A^T with S = A); small_layout 1: S is stored [K][r] (v = dy B with S = B, K standing for the layer's N).
 * dinox_lora_up:    t[M][N] (fp32) = s . u[M][r] . S (+ res[M][N] fp32, NULL: none; res == t is allowed).  small_layout 0: S is stored [N][r]
 *   (the forward term, S = B); small_layout 1: S is stored [r][N] (the dX term s (v A), S = A and N standing for the layer's K).
 * dinox_lora_grad:  dA[r][K] = s v^T xl and dB[N][r] = s dy^T u with u = xl A^T, v = dy B formed on chip, xl and dy read once from memory.
 *   Workgroup c takes rows [128 c, 128 c + 128), writes its partial sums to ws (dinox_lora_grad_ws_bytes(M, K, N, r) bytes, contents need not
 *   be initialised); a second launch adds the partials in ascending c and applies s.  Nothing outside dA, dB and that many bytes of ws is written.
 * dinox_lora_dropout: out[i] = keep(i) ? in[i] / (1 - p) : 0 for i < n, 0 <= p < 1, in == out allowed.  No mask is stored:
 *   keep(i) = (h(i) >> 8) >= ceil(p 2^24),   h(i) = mix(lo32(i) ^ mix(hi32(i) + key)),
 *   key = mix(lo32(offset) ^ mix(hi32(offset) + mix(lo32(seed) ^ mix(hi32(seed) + 0x9e3779b9)))),   all in uint32 arithmetic,
 *   mix(x): x ^= x >> 16; x *= 0x21f0aaad; x ^= x >> 15; x *= 0x735a2d97; x ^= x >> 15.
 * dinox_lora_merge: w_out[N][K] (fp32) = w[N][K] + sign . s . B A, sign = +1 (merge) or -1 (unmerge); w_out == w is allowed.
 * ------------------------------------------------------------------------------------------ */
int dinox_lora_down(const void* x, const float* small, float* u, int64_t M, int K, int r, int small_layout, int dtype, void* stream);
int dinox_lora_up(const float* u, const float* small, const float* res, float* t, float s, int64_t M, int N, int r, int small_layout,
                  void* stream);
int64_t dinox_lora_grad_ws_bytes(int64_t M, int K, int N, int r);
int dinox_lora_grad(const void* xl, const void* dy, const float* A, const float* B, float s, float* dA, float* dB, float* ws, int64_t M, int K,
                    int N, int r, int dtype, void* stream);
int dinox_lora_dropout(const void* in, void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, void* stream);
int dinox_lora_merge(const float* w, const float* A, const float* B, float* w_out, float s, int sign, int N, int K, int r, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense segmentation loss on patch logits (kernels: csrc/segloss.hip; autograd node: dinox.ops.SegLossFn).  A linear head gives one
 * logit row per patch; the loss is taken at full resolution, and no tensor of B C S^2 elements is written in either direction.
 *   z[B][P][C]  fp32, dense, P = g^2, patch i = gy g + gx.  2 <= C <= 64 (C > 64: DINOX_EUNSUPPORTED; C < 2: DINOX_EINVAL).
 *   y[B][S][S]  uint8, S = g u, 1 <= u <= 32 (the patch size).  255 = ignore.  Any other value >= C is an argument error: such a pixel
 *               is left out like an ignored one (a label is only ever compared, never an address), and the calls COUNT them -- nv[1] of
 *               the forward, counts[3 C] of predict -- for the caller to refuse.
 *   l_p[c]      bilinear upsampling, align_corners = False: along x the source coordinate is s = max((x + 0.5) / u - 0.5, 0),
 *               x0 = floor(s), x1 = min(x0 + 1, g - 1), the weight of x1 is s - x0; y alike; l_p is the 4-tap interpolation of z.
 *   p_p = softmax(l_p) (max subtracted);  Nv = number of pixels with y_p != 255 (and < C);
 *   CE = (1 / Nv) sum_valid (lse(l_p) - l_p[y_p]);
 *   I_c = sum_valid p_pc [y_p = c],  P_c = sum_valid p_pc,  Y_c = sum_valid [y_p = c]   (over the whole batch);
 *   D_c = (2 I_c + 1) / (P_c + Y_c + 1);   Dice = 1 - mean_{c >= c0} D_c,  c0 in {0, 1} (1: the background class is left out);
 *   L = w_ce CE + w_dice Dice.   Nv = 0: every loss is 0 and every gradient exactly 0.
 *   G_pc = (w_ce / Nv)(p_pc - [y_p = c]) + w_dice p_pc (a_pc - sum_k p_pk a_pk),
 *   a_pc = -(1 / (C - c0)) (2 [y_p = c](P_c + Y_c + 1) - (2 I_c + 1)) / (P_c + Y_c + 1)^2 for c >= c0, 0 below;  G = 0 at ignored pixels;
 *   dz[b][j][c] = grad_scale sum_p W(p, j) G_pc,  W(p, j) = the bilinear weight of patch j at pixel p.
 * Every entry checks its arguments on the host (a message before any launch), allocates nothing and does not synchronise.  Floating-point
 * sums have a fixed order (per lane, wave butterfly, partial sums in the workspace added in ascending order by a second launch): equal
 * inputs give equal bits.  Integer counts use integer atomics.  1 <= B <= 2^20, 1 <= g <= 4096, B g^2 <= 2^32.
 *
 * dinox_seg_loss_ws_bytes: bytes of workspace for forward and backward (a pure function of the sizes; 0 for sizes the calls refuse; contents
 *   need not be initialised; 4-byte aligned).
 * dinox_seg_loss_fwd: loss[3] = (L, CE, Dice) fp32, stats[3][C] = (I, P, Y) fp32, nv[2] = (Nv, number of labels >= C other than 255).
 * dinox_seg_loss_bwd: dz[B][P][C] fp32 from z, y and the forward's stats and nv (device pointers; nothing crosses to the host).
 * dinox_seg_predict:  pred[B][S][S] uint8 = argmax_c l_p[c], the lowest index on an exact tie.  y != NULL (then counts != NULL, and both or
 *   neither): counts[3 C + 1] int64 = per class the true positives, the predicted pixels and the labelled pixels over the valid pixels,
 *   then the number of labels >= C other than 255.  counts is zeroed on the stream first.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_seg_loss_ws_bytes(int64_t B, int g, int u, int C);
int dinox_seg_loss_fwd(const float* z, const uint8_t* y, float* loss, float* stats, int64_t* nv, void* ws, int64_t B, int g, int u, int C,
                       int c0, float w_ce, float w_dice, void* stream);
int dinox_seg_loss_bwd(const float* z, const uint8_t* y, const float* stats, const int64_t* nv, float* dz, void* ws, int64_t B, int g, int u,
                       int C, int c0, float w_ce, float w_dice, float grad_scale, void* stream);
int dinox_seg_predict(const float* z, const uint8_t* y, uint8_t* pred, int64_t* counts, int64_t B, int g, int u, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * Calibration of a dense segmenter (kernel: csrc/segcalib.hip; dinox.ops.seg_calib, dinox.segment.calibration_report / fit_temperature).
 * z, y, the geometry, the limits and the interpolated logits l_p[c] are those of the section above (same weights, same order of
 * operations).  s = inv_temperature, finite and > 0.  Per pixel p, one launch over the patch logits, nothing of full resolution but the
 * requested maps:
 *   pred    = argmax_c l_p[c], lowest index on an exact tie, taken on the UNSCALED logits: dinox_seg_predict's map bit for bit, whatever s;
 *   t_c     = s l_p[c] (one fp32 multiply);  p = softmax(t) (max subtracted);  lse = log sum_c exp(t_c);
 *   conf    = p[pred];
 *   entropy = (lse - sum_c p_c t_c) fl(1 / log C), clamped to [0, 1] by comparisons (a NaN stays NaN).  A class of probability 0 adds 0 to
 *             this and every other p-weighted sum (also where its logit is -inf).
 * pred[B][S][S] uint8, conf and entropy [B][S][S] fp32: each may be NULL; written for every pixel, ignored ones included.
 * y != NULL (then hist, sums and ws are non-NULL, and NULL with y == NULL: all four or none): statistics over the VALID pixels, y_p != 255
 * and y_p < C.
 *   hist[3 NB + 3] int64, zeroed on the stream first, 1 <= NB <= 64.  A valid pixel with finite conf falls into bin
 *     k = min((int)(conf * (float)NB), NB - 1) (one fp32 multiply; the index is clamped by comparisons before it addresses anything) and
 *     hist[3 k + (0, 1, 2)] += (1, [pred = y_p], q) with q = (int64)rintf(conf * 16777216.f), the confidence in 2^-24 fixed point.
 *     hist[3 NB + (0, 1, 2)] = Nv, the number of labels >= C other than 255, the number of valid pixels whose conf is not finite (these
 *     enter no bin and no sum).  All integers, integer atomics: exact and independent of the order.
 *   sums[5] fp32 over the valid pixels with finite conf:
 *     NLL = sum (lse - t_y);  Brier = sum sum_c (p_c - [y_p = c])^2;  G = sum (mu - l_y) with mu = sum_c p_c l_c (= d NLL / d s);
 *     H = sum sum_c p_c (l_c - mu)^2 (= d^2 NLL / d s^2 >= 0);  sum entropy.
 *     Fixed order (per lane in row order, wave butterfly, partial sums in ws by plain stores, a second launch adds them ascending): equal
 *     inputs give equal bits.  No floating-point atomic.
 * Argument checks on the host with a message before any launch (DINOX_EINVAL: NB outside [1, 64], s not finite or <= 0, pointers that
 * break the all-or-none rule, nothing to compute); no allocation, no synchronisation.
 * dinox_seg_calib_ws_bytes: bytes of workspace (a pure function of the sizes; 0 for sizes the call refuses; contents need not be
 *   initialised; 4-byte aligned).
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_seg_calib_ws_bytes(int64_t B, int g, int u, int C, int NB);
int dinox_seg_calib(const float* z, const uint8_t* y, float inv_temperature, uint8_t* pred, float* conf, float* entropy, int64_t* hist,
                    float* sums, void* ws, int64_t B, int g, int u, int C, int NB, void* stream);

/* ------------------------------------------------------------------------------------------
 * Edge-aware label refinement: mean-field iterations of a local CRF on a guide image (kernel: csrc/segrefine.hip; dinox.ops.seg_refine,
 * dinox.segment.RefineConfig).  Inputs: patch logits z[B][g g][C] fp32, with geometry (B, g, u, C) and limits exactly those of
 * dinox_seg_predict; a guide image I[B][S][S] fp32, with S = g u; the scalars s (inverse temperature, finite and > 0), T (iterations,
 * 0...32), r (window radius, 1...3), d (dilation, 1...8), sigma_xy > 0 in pixels of the S-grid, sigma_I > 0 in units of I, lambda in
 * [0, 1], w >= 0, finite.  With l_p[c] the interpolated logit of seg_common.h (same taps, same order of operations):
 *   U_p[c]    = s l_p[c]                                   (one fp32 multiply)
 *   Q^0_p     = softmax_c(U_p)                             (max subtracted)
 *   N(p)      = { p + d (dy, dx) : |dy|, |dx| <= r, (dy, dx) != (0, 0), inside the image }
 *   g_(dy,dx) = exp(-(dy^2 + dx^2) d^2 / (2 sigma_xy^2))   (host-computed fp32 table of (2r+1)^2 entries, passed to the kernel)
 *   a_pj      = (1 - lambda) + lambda exp(-(I_p - I_j)^2 / (2 sigma_I^2))
 *   m_p[c]    = sum_{j in N(p)} g_pj a_pj Q^(t-1)_j[c]  /  sum_{j in N(p)} g_pj
 *   Q^t_p     = softmax_c(U_p[c] + w m_p[c])               t = 1...T
 * The normaliser is the spatial sum over the neighbours inside the image: the appearance term can only weaken a message, never strengthen
 * it.  The neighbour sum runs in a fixed order: dy outer, dx inner, ascending; equal inputs give equal bits.  Out-of-image neighbours
 * contribute to neither sum.  r d >= S in an axis, which leaves no neighbour, is refused; so is 2 d > S, which leaves the pixels with
 * S - d <= x < d and S - d <= y < d no neighbour at any radius (with 2 d <= S every pixel keeps p + (0, d) or p - (0, d): N(p) is never
 * empty and no normaliser is 0).
 * Outputs: pred[B][S][S] uint8 = arg-max of Q^T, taken on the pre-softmax values U + w m, lowest index on an exact tie; optional
 * conf[B][S][S] fp32 = Q^T[pred]; optional y / counts[3 C + 1], exactly as dinox_seg_predict does it (of the refined map; both or neither).
 * With T = 0, pred and counts are dinox_seg_predict's bit for bit (the arg-max is then taken on the unscaled l_p, as dinox_seg_calib takes
 * it) and conf is dinox_seg_calib's at the same s.
 * The kernel receives gtab (a HOST pointer to the (2r+1)^2 values g_(dy,dx), row-major, dy outer; the centre is not read; copied into the
 * launch arguments) and inv2sI2 = 1 / (2 sigma_I^2).  ws: two ping-pong planes Q[B][C][S][S] fp32 (class-major), needed when T >= 1.
 * One launch writes Q^0, one launch runs each iteration; the last iteration writes no plane and produces pred, conf and counts itself.
 * A non-finite logit or guide pixel does not fault: it makes non-finite every value whose windows it enters, and nothing else.
 * Host checks before any launch (DINOX_EINVAL with a message): the geometry, T, r, d, r d >= S, 2 d > S, s / w / inv2sI2 / lambda / gtab not finite or
 * out of range (gtab >= 0, and > 0 at the four nearest neighbours so that no normaliser is 0), null z, I, pred or gtab, y without counts
 * or counts without y, T >= 1 without ws.  No allocation, no synchronisation.
 * dinox_seg_refine_ws_bytes: bytes of the two planes (a pure function of the sizes; 0 for sizes the call refuses, among them more than
 *   2^31 - 1 tiles of 32 x 8 pixels or more than 2^40 elements per plane; contents need not be initialised; 4-byte aligned).
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_seg_refine_ws_bytes(int64_t B, int g, int u, int C);
int dinox_seg_refine(const float* z, const float* I, const uint8_t* y, uint8_t* pred, float* conf, int64_t* counts, void* ws, int64_t B, int g,
                     int u, int C, int T, int r, int d, const float* gtab, float inv2sI2, float lambda, float w, float s, void* stream);

/* ------------------------------------------------------------------------------------------
 * Sliding-window prediction at native resolution (kernel: csrc/segblend.hip; dinox.ops.seg_blend_predict, dinox.tiled).  B images of one
 * size H x W were cut into t x t tiles on a separable grid of origins ys[ny] x xs[nx]; every tile went through the model F times (mirror
 * variants) and left g x g patch logit rows.  Each output pixel gathers the tiles that cover it: no [C][H][W] map is written, nothing is
 * scattered, and there is no floating-point atomic.
 *   z[B][F][ny][nx][g g][C]  fp32, dense.  2 <= C <= 64 (C > 64: DINOX_EUNSUPPORTED).  1 <= F <= 4.
 *   ys[ny], xs[nx]  device int32, ascending tile origins, 0 <= ys[i] <= H - t, 0 <= xs[i] <= W - t.  The kernel TRUSTS both tables (the
 *               caller checks its host copies); a pixel that no tile covers gets label 0 and a NaN confidence.
 *   flips[F]    device int32: bit 0 = the model saw the tile mirrored along x, bit 1 = along y.
 *   win[t]      device fp32, the 1-D window: tile pixel (ly, lx) weighs w = win[ly] win[lx] (one fp32 product; the kernel evaluates no
 *               window function, the host rounds it once).
 *   Per pixel (y, x), variant f and covering tile (iy, ix):  ly = y - ys[iy], mirrored to t - 1 - ly if flips[f] & 2;  lx alike with
 *               bit 0.  Along each axis the patch coordinate is s = max((l + 0.5) g / t - 0.5, 0), taps k = floor(s) and min(k + 1, g - 1),
 *               the weight of the second tap is the integer (2 l + 1) g - t - 2 t k over 2 t (0 where s was clamped or the second tap is
 *               clamped onto the first): bilinear, align_corners = False, for any t >= 1.  l_c = the 4-tap interpolation, x first.
 *   L_c = (sum w l_c) / (sum w), both sums over f, then iy, then ix, all ascending, in fp32;  one division per class.
 *   pred[B][H][W] uint8 = argmax_c L_c, the lowest index on an exact tie; always < C, whatever the bits of z.
 *   conf[B][H][W] fp32 (or NULL) = 1 / sum_c exp(L_c - max_c L_c).
 *   y[B][H][W] uint8 or NULL (then counts NULL too: both or neither): counts[3 C + 1] int64 exactly as dinox_seg_predict's.
 * Equal inputs give equal bits.  T = B F ny nx >= 1, 1 <= g <= 4096, 1 <= t <= min(H, W), H, W <= 2^20, B <= 2^20 and B H ceil(W / 64)
 * <= 2^32; anything else, or a null pointer, is DINOX_EINVAL with a message before any launch.
 * ------------------------------------------------------------------------------------------ */
int dinox_seg_blend_predict(const float* z, const int32_t* ys, const int32_t* xs, const int32_t* flips, const float* win, const uint8_t* y,
                            uint8_t* pred, float* conf, int64_t* counts, int64_t B, int F, int ny, int nx, int g, int t, int C, int H, int W,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Patch sampling for segmentation training at native resolution (kernel: csrc/segpatch.hip; dinox.ops.seg_patch_sample, dinox.patches).
 * One launch turns B jobs into the image batch x[B][3][S][S] fp32 and the label batch m[B][S][S] uint8.  Both are sampled from a
 * device-resident pool under the job's inverse affine map; the source point is computed once per output pixel and serves both.
 *   img         fp32 planes, already windowed to [0, 1];  msk  uint8 planes.  A plane is H x W, contiguous.
 *   jobs[B][4]  device int64 = {element offset of the image plane in img, element offset of the mask plane in msk, H, W}, 1 <= H, W <= 2^20.
 *               Planes of different sizes may meet in one launch; offsets carry no alignment promise.  The kernel TRUSTS jobs (the caller
 *               checks its host copy against the sizes of the pools).
 *   par[B][8]   device fp32 = {a00, a01, a02, a10, a11, a12, gamma, gain}, finite, gamma > 0 (the caller's check; see Safety).
 *   Coordinates.  Output pixel (oy, ox) has dx = ox + 0.5 - S / 2 and dy = oy + 0.5 - S / 2 (exact in fp32), and
 *               sx = fmaf(a00, dx, fmaf(a01, dy, a02)),   sy = fmaf(a10, dx, fmaf(a11, dy, a12))
 *               in fp32, in exactly this order: a CPU fp32 emulation reproduces sx and sy to the bit.  Source pixel i covers [i, i + 1).
 *   Label.      m = msk[floor(sy)][floor(sx)] if 0 <= sx < W and 0 <= sy < H, else 255 (the ignore value of the loss kernels: padding
 *               never trains).
 *   Image.      Bilinear at u = sx - 0.5, v = sy - 0.5 (one fp32 subtraction each): taps floor(u), floor(u) + 1 with weights 1 - wx, wx,
 *               wx = u - floor(u) (exact); rows alike; x first.  A tap outside the plane takes `pad`; a point with u <= -1, u >= W,
 *               v <= -1 or v >= H (every tap outside) gives exactly `pad`.  Then v' = gain max(v, 0)^gamma, the power (powf) and its
 *               clamp skipped when gamma == 1, so that the identity job is exact; then x_c = (v' - mean_c) / std_c for c = 0, 1, 2 (the one
 *               plane replicated), an IEEE subtraction and division.  mean, std: HOST arrays of 3 floats read during the call, std > 0.
 *   Safety.     No content of par moves an access: a coordinate is compared with the plane's bounds in fp32 BEFORE any conversion to an
 *               integer (a NaN or a huge value is outside), and every tap index is used only after 0 <= i < W (or H) was tested.
 * Plain stores, no atomics, no LDS: equal inputs give equal bytes.  1 <= S <= 2^14, 1 <= B <= 2^20 and B S ceil(S / 64) <= 2^31; anything
 * else, a null pointer, a non-finite mean, std or pad, or std <= 0 is DINOX_EINVAL with a message before any launch.  The entry allocates
 * nothing and does not synchronise.  No antialiasing when a job shrinks the source.
 * ------------------------------------------------------------------------------------------ */
int dinox_seg_patch_sample(const float* img, const uint8_t* msk, const int64_t* jobs, const float* par, float* x, uint8_t* m, int64_t B, int S,
                           const float* mean, const float* stdev, float pad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Surface distances between two label maps, in mm (kernels: csrc/surfdist.hip; dinox.ops.surface_stats, dinox.segment.surface_metrics).
 *   pred[B][H][W], gt[B][H][W]  uint8, dense, 1 <= H, W <= 1024 (rectangular maps are fine: nothing here knows a patch grid), B >= 1 and
 *               B C 2 H <= 2^30.  Classes 0 .. C - 1, 2 <= C <= 64.  gt == 255 is ignore.  A pred value >= C, or a gt value >= C other
 *               than 255, is an argument error: it belongs to no class (a label is only ever compared, never an address) and the call
 *               COUNTS them -- bad[0] for pred, bad[1] for gt -- for the caller to refuse.
 *   spacing[B][2]  fp32 on the device, (s_y, s_x) in mm per pixel of each image, finite and > 0.
 *   Sets, per image b and class c:  A = {p : gt_p != 255 and pred_p = c},  G = {p : gt_p = c}; an ignored pixel is in neither.
 *   Border dX of a set X: the pixels of X with at least one of their four edge neighbours outside X; a neighbour outside the image is
 *               outside X (X and not binary_erosion(X) with the 4-connected cross).
 *   d(p, Y) = min over q in Y of sqrt((s_y (p_y - q_y))^2 + (s_x (p_x - q_x))^2).
 *   Directed surface distances: D_AG = {d(p, dG) : p in dA} (direction 0), D_GA = {d(p, dA) : p in dG} (direction 1).
 *   Per (b, c, direction):  n = the number of border pixels on the query side; the sum and the maximum of the distances; the k-th smallest
 *               distance, k = ceil(n q_num / q_den) in integer arithmetic (nearest rank; 0 < q_num <= q_den, e.g. 95 / 100; n = 20 gives
 *               k = 19); for each of T tolerances tol_t (1 <= T <= 8, mm, finite, >= 0) the number of distances <= tol_t.
 *               If either border is empty the three floats and the T tolerance counts are 0; n of the two directions says which side was.
 *   HD95 = max of the two quantiles, HD = max of the two maxima, ASSD = (sum_AG + sum_GA) / (n_A + n_G),
 *   NSD(tol) = (within_AG + within_GA) / (n_A + n_G) are formed by the caller (dinox.segment.surface_metrics).
 * An exact separable distance transform: a column scan (vertical distance in pixels to the nearest border pixel of the column), a row
 * minimum over (s_x (x - x'))^2 + (s_y d)^2 at the border pixels only, then per (b, c, direction) a reduction and a radix select on the
 * fp32 bit patterns.  A distance is sqrt(fl(fl(s_x k)^2 + fl(s_y m)^2)), every operation rounded once: within 3 * 2^-24 of the exact
 * one, relatively.  The sum has a fixed order (per lane, wave butterfly, per-wave partials in ascending order); maximum, counts and
 * the select are integer work: equal inputs give equal bits, and an image's outputs do not depend on the rest of the batch.
 * The entry checks its arguments on the host (a message before any launch), allocates nothing and does not synchronise.
 *
 * dinox_surface_ws_bytes: bytes of workspace, 12 B C H W (a pure function of the sizes; 0 for sizes the call refuses; contents need not
 *   be initialised; 4-byte aligned).
 * dinox_surface_stats: counts[B][C][2][1 + T] int64 = (n, within tol_0 .. tol_{T-1}); values[B][C][2][3] fp32 = (sum, max, quantile);
 *   bad[2] int64, zeroed on the stream first.  tol is a HOST array of T floats, read during the call; every other pointer is a device
 *   pointer.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_surface_ws_bytes(int64_t B, int H, int W, int C);
int dinox_surface_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values,
                        int64_t* bad, void* ws, int64_t B, int H, int W, int C, int T, int q_num, int q_den, void* stream);

/* ------------------------------------------------------------------------------------------
 * Surface distances between two label VOLUMES, in mm (kernels: csrc/surfdist3d.hip; dinox.ops.surface_stats_3d,
 * dinox.segment.surface_metrics_3d).  One volume per call; everything is as in the section above with these differences:
 *   pred[Z][H][W], gt[Z][H][W]  uint8, dense, 1 <= Z, H, W <= 1024 (an axis distance fits uint16 beside its sentinel, one axis line fits
 *               LDS), hence Z H W <= 2^30 as the 3-D components have it (every n fits an unsigned 32-bit integer).  Classes 0 .. C - 1, 2 <= C <= 64.  gt == 255 is
 *               ignore.  Bad values are counted as above: bad[0] pred values >= C, bad[1] gt values >= C other than 255.
 *   spacing[3]  fp32, a HOST array read during the call: the voxel (s_z, s_y, s_x) in mm, finite and > 0.
 *   Sets, per class c:  A = {p : gt_p != 255 and pred_p = c},  G = {p : gt_p = c}; an ignored voxel is in neither.
 *   Border dX of a set X: the voxels of X with at least one of their SIX FACE NEIGHBOURS outside X; a neighbour outside the volume is
 *               outside X (X and not binary_erosion(X) with the 6-connected cross, the default structuring element of scipy and MedPy in
 *               3-D).  A volume with Z = 1 therefore has dX = X: both z neighbours of every voxel are outside.  That is intended, and it
 *               is NOT the 2-D result of the section above for the same slice.
 *   d(p, Y) = min over q in Y of sqrt((s_z (p_z - q_z))^2 + (s_y (p_y - q_y))^2 + (s_x (p_x - q_x))^2).
 *   Directed distances, n, sum, maximum, the k-th smallest with k = ceil(n q_num / q_den) in integers, the T tolerance counts and the
 *               rule for an empty border are those of the section above; HD95, HD, ASSD and NSD are formed by the caller
 *               (dinox.segment.surface_metrics_3d).
 * An exact separable distance transform in three axis passes, one class at a time over the same planes: a z scan (distance in voxels to
 * the nearest border voxel of the z column, uint16), a y minimum over (s_y (y - y'))^2 + (s_z d)^2 at every voxel, an x minimum over
 * (s_x (x - x'))^2 + that value at the query border voxels only, then a reduction per slice, four digit histograms of a radix select on
 * the fp32 bit patterns spread over the slices (integer atomics in global memory) and one workgroup that adds the slice sums in ascending
 * z.  A distance is sqrt(fl(fl(fl(s_x k)^2) + fl(fl(fl(s_y m)^2) + fl(fl(s_z n)^2)))), every operation rounded once: each square is
 * within (1 + u)^3 of exact, the inner sum (1 + u)^4, the radicand (1 + u)^5, its correctly rounded root within 2.5 u + u = 3.5 u of the
 * exact distance, relatively (u = 2^-24).  No floating-point atomics; equal inputs give equal bits whatever the workspace held.
 * The entry checks its arguments on the host (a message before any launch), allocates nothing and does not synchronise.
 *
 * dinox_surface3d_ws_bytes: bytes of workspace, 12 Z H W + 8 Z + 8320 -- two uint16 planes of z distances, two fp32 planes that hold the
 *   squared y-z distances and then the distances, 2 Z slice sums and 8320 bytes of counters and histograms; C does not enter (a pure
 *   function of the sizes; 0 for sizes the call refuses; contents need not be initialised; 4-byte aligned).
 * dinox_surface3d_stats: counts[C][2][1 + T] int64 = (n, within tol_0 .. tol_{T-1}); values[C][2][3] fp32 = (sum, max, quantile);
 *   direction 0 runs from dA to dG, 1 the other way; bad[2] int64, zeroed on the stream first.  spacing and tol are HOST arrays of 3 and
 *   T floats, read during the call; every other pointer is a device pointer.
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_surface3d_ws_bytes(int64_t Z, int H, int W, int C);
int dinox_surface3d_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values,
                          int64_t* bad, void* ws, int64_t Z, int H, int W, int C, int T, int q_num, int q_den, void* stream);

/* ------------------------------------------------------------------------------------------
 * Boundary loss: the signed distance map of a label map and the boundary term of the dense segmentation loss (Kervadec et al., MIDL
 * 2019; kernels: csrc/distmap.hip and the *_bd_* kernels of csrc/segloss.hip; dinox.ops.signed_distance_map, dinox.ops.SegBoundaryLossFn).
 *
 * Signed distance map.
 *   y[B][H][W]  uint8, dense, 1 <= H, W <= 1024 (rectangular maps are fine), B >= 1 and B C H <= 2^30.  Classes 0 .. C - 1, 2 <= C <= 64
 *               (C > 64: DINOX_EUNSUPPORTED; C < 2: DINOX_EINVAL).  255 is ignore.  A value >= C other than 255 is an argument error: it
 *               belongs to no set (a label is only ever compared, never an address) and the call COUNTS them -- bad[0] -- for the caller
 *               to refuse.
 *   spacing[B][2]  fp32 on the device, (s_y, s_x) per pixel of each image (mm, or 1 for distances in pixels), finite and > 0.
 *   Sets, per image b and class c:  G = {p : y_p = c},  R = {p : y_p != c, y_p != 255, y_p < C}; an ignored pixel is in neither and is
 *               never a source.
 *   d(p, X) = min over q in X of sqrt((s_y (p_y - q_y))^2 + (s_x (p_x - q_x))^2), between pixel centres.
 *   phi_c(p) = +d(p, G) for p in R,  -d(p, R) for p in G,  0 at ignored pixels, and 0 wherever the set the pixel needs is empty (the class
 *               is absent from the image, or covers every valid pixel of it).
 *   Nothing outside the image counts as outside the class (unlike the border of the surface metrics above): an organ cut by the crop has
 *               no boundary at the image edge.  Without ignored pixels phi_c is
 *               distance_transform_edt(~G, sampling) * ~G - distance_transform_edt(G, sampling) * G of scipy.ndimage.
 * The exact separable transform of the surface kernels, dense: a column scan (per pixel the vertical distance in pixels to the nearest G
 * and to the nearest R pixel of its column, two uint16 planes), then per row the minimum over x' of (s_x (x - x'))^2 + (s_y d)^2 against
 * the plane the pixel's own membership selects, the square root and the sign.  A distance is sqrt(fl(fl(s_x k)^2 + fl(s_y m)^2)), every
 * operation rounded once: within 3 * 2^-24 of the exact one, relatively.  There are no sums and no floating-point atomics: equal inputs
 * give equal bits, an image's planes do not depend on the rest of the batch, nor a class's plane on C beyond which pixels are valid.
 *
 * Boundary term.  z, y, the bilinear upsampling, p = softmax, Nv and c0 are those of the dense segmentation loss above; phi[B][C][S][S] fp32
 * as produced here (the planes below c0 are not read).
 *   BD = (1 / (Nv (C - c0))) sum_valid sum_{c >= c0} p_pc phi_c(p);   L = w_ce CE + w_dice Dice + w_bd BD.
 *   G_pc gains (w_bd / (Nv (C - c0))) p_pc (phi_pc - sum_{k >= c0} p_pk phi_pk), phi_pk = 0 for k < c0: the Dice term's p (a - sum p a)
 *   with a per-pixel a, so it rides the same pixel pass -- one softmax per pixel per direction, no further launch over the pixels.
 *   BD can be negative (a good prediction sits inside its region).  Nv = 0: BD = 0 and the gradient is exactly 0.  With w_bd = 0 the
 *   calls return L, CE, Dice, stats and dz bit-equal to dinox_seg_loss_fwd / _bwd -- they run those very kernels, and the forward reports
 *   BD from a launch of the boundary kernels of its own (the one case with a second launch over the pixels; nothing trains on it).
 * Every entry checks its arguments on the host (a message before any launch), allocates nothing and does not synchronise; sums keep the
 * fixed order of the section above.
 *
 * dinox_signed_distance_ws_bytes: bytes of workspace, 4 B C H W -- the two uint16 planes (a pure function of the sizes; 0 for sizes the call
 *   refuses; contents need not be initialised; 4-byte aligned).
 * dinox_signed_distance: phi[B][C][H][W] fp32, dense; bad[1] int64, zeroed on the stream first.  Every pointer is a device pointer.
 * dinox_seg_loss_bd_ws_bytes: as dinox_seg_loss_ws_bytes, one float more per partial sum of the forward.
 * dinox_seg_loss_bd_fwd: loss[4] = (L, CE, Dice, BD) fp32; stats and nv as dinox_seg_loss_fwd.
 * dinox_seg_loss_bd_bwd: dz[B][P][C] fp32 from z, y, phi and the forward's stats and nv.
 * ------------------------------------------------------------------------------------------ */
size_t dinox_signed_distance_ws_bytes(int64_t B, int H, int W, int C);
int dinox_signed_distance(const uint8_t* y, const float* spacing, float* phi, int64_t* bad, void* ws, int64_t B, int H, int W, int C,
                          void* stream);
size_t dinox_seg_loss_bd_ws_bytes(int64_t B, int g, int u, int C);
int dinox_seg_loss_bd_fwd(const float* z, const uint8_t* y, const float* phi, float* loss, float* stats, int64_t* nv, void* ws, int64_t B,
                          int g, int u, int C, int c0, float w_ce, float w_dice, float w_bd, void* stream);
int dinox_seg_loss_bd_bwd(const float* z, const uint8_t* y, const float* phi, const float* stats, const int64_t* nv, float* dz, void* ws,
                          int64_t B, int g, int u, int C, int c0, float w_ce, float w_dice, float w_bd, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of a label map: labelling, clean-up and lesion-wise matching (kernels: csrc/cclabel.hip; dinox.ops.cc_label,
 * cc_filter, lesion_counts; dinox.segment.postprocess, lesion_metrics).
 *   labels[B][H][W]  uint8, dense, 1 <= H, W <= 1024 (rectangular is fine), B >= 1 and B H W < 2^31.  Classes 0 .. C - 1, 2 <= C <= 64.
 *   mask[B][H][W]    uint8 or NULL.  A pixel whose mask value is 255 belongs to no component (pass the ground truth to restrict a
 *               prediction to the pixels the ground truth does not ignore: the set A of the surface-distance section).
 *   A pixel whose label is >= C belongs to no component.  255 in labels is simply such a pixel; any other value >= C at a pixel the mask
 *               does not exclude is an argument error, which the call COUNTS (bad[0]) for the caller to refuse: a label is only ever
 *               compared, never an address.
 *   Neighbours: connectivity 4, the pixels that share an edge; connectivity 8, an edge or a corner.  Two pixels are joined when they are
 *               neighbours, both belong to a component and carry the same class value.  A component is a maximal joined set.  Every class is
 *               labelled in the one pass, background (class 0) included.
 *   Canonical form: comp[B][H][W] int32 = the linear index y W + x, inside its image, of the component's first pixel in raster order (its
 *               smallest index, its ROOT), -1 where the pixel is in no component.  It is unique, so two labellings compare bit for bit.
 *               area[B][H][W] int32 = the component's pixel count at its root pixel, 0 everywhere else.
 *               ncomp[B][C] int64 = the number of components per image and class.
 *   Filter: out[B][H][W] uint8 = labels where the pixel's component is kept, 0 where it is removed or the pixel is in none.  Classes below
 *               c0 (0 <= c0 <= C; 1 keeps the background whatever its shape) are always kept.  A component of a class >= c0 is kept iff its
 *               area >= min_px[b] and, with keep_largest != 0, it is also the largest of its (image, class).  Tie rule: of components with
 *               equal area the one with the SMALLEST root index is the largest (one 64-bit maximum over area << 20 | (2^20 - 1 - root)).
 *               The largest is chosen among all components of the class, whatever min_px says.  min_px: device int32 [B], or NULL for 1.
 *               y != NULL (then counts != NULL, both or neither): counts[3 C + 1] int64 of out against y, exactly dinox_seg_predict's:
 *               per class the true positives, the predicted pixels and the labelled pixels over the pixels with y != 255, then the
 *               number of y values >= C other than 255 (such a pixel counts nowhere else).  Zeroed on the stream first.
 *   Match: a prediction and a ground truth with the comp / area of each, the prediction labelled with mask = gt.  Every pixel p with
 *               pred_p = gt_p = c inside a component on both sides adds 1 to `inter` of its pred component and of its gt component.
 *               A component with area < min_px[b] is not a lesion on its side; its pixels still count as overlap for the other side.
 *               Hit criterion, per component: inter >= 1 and inter t_den >= t_num area, in int64; 0 <= t_num <= t_den, 0 < t_den < 2^20;
 *               t_num = 0: any overlap.  counts[B][C][4] int64 = (n_gt, n_gt_hit, n_pred, n_pred_hit), zeroed on the stream first.
 *               The criterion is per component: no pair table.  Sensitivity = n_gt_hit / n_gt, precision = n_pred_hit / n_pred
 *               (dinox.segment.lesion_metrics).
 * Labelling is union-find with parent <= child throughout, so a root is its component's smallest index: a workgroup per 32 x 32 tile in
 * LDS, then a launch that unites across tile edges (and corners for connectivity 8) with agent-scope atomics on the parent array, then a
 * launch that gives every pixel its root and counts.  No loop waits for another wave: each is bounded by strictly decreasing indices or
 * by the 64 lanes of a wave.  All of it is integer work: equal inputs give equal bits, and an image's outputs do not depend on the batch.
 * Every entry checks its arguments on the host (a message before any launch), allocates nothing, reads nothing back and does not
 * synchronise.
 *
 * dinox_cc_ws_bytes: bytes of workspace for any of the three calls, 8 B H W + 8 B C (a pure function of the sizes; 0 for sizes the calls
 *   refuse; contents need not be initialised; 8-byte aligned).
 * dinox_cc_label: connectivity 4 or 8; bad[1] int64, zeroed on the stream first.
 * dinox_cc_filter: comp / area as dinox_cc_label wrote them for `labels` (same mask, same connectivity).
 * dinox_cc_match: pred_comp / pred_area from dinox_cc_label(pred, mask = gt), gt_comp / gt_area from dinox_cc_label(gt, mask = NULL).
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_cc_ws_bytes(int64_t B, int H, int W, int C);
int dinox_cc_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t B,
                   int H, int W, int C, int connectivity, void* stream);
int dinox_cc_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, const uint8_t* y, uint8_t* out,
                    int64_t* counts, void* ws, int64_t B, int H, int W, int C, int c0, int keep_largest, void* stream);
int dinox_cc_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                   const int32_t* gt_area, const int32_t* min_px, int64_t* counts, void* ws, int64_t B, int H, int W, int C, int t_num, int t_den,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Connected components of ONE label volume: the calls above for a series instead of a batch of independent images (kernels:
 * csrc/cclabel3d.hip on the stages of csrc/cclabel.hip; dinox.ops.cc_label_3d, cc_filter_3d, lesion_counts_3d;
 * dinox.segment.segment_volume, postprocess_volume).  Everything is as in the section above with these differences:
 *   labels[Z][H][W]  uint8, dense, 1 <= H, W <= 1024, Z >= 1 and Z H W <= 2^30 (every voxel index and every area fits int32).  mask likewise.
 *   Neighbours: connectivity 6, the voxels that share a face; 18, a face or an edge; 26, a face, an edge or a corner.
 *   Canonical form: comp[Z][H][W] int32 = the linear index (z H + y) W + x of the component's first voxel in raster order, -1 where the
 *               voxel is in no component; area[Z][H][W] int32 = the voxel count at the root, 0 elsewhere; ncomp[C] int64.
 *   Filter: min_vox is a host scalar >= 0 (one volume, one minimum).  Tie rule: of components with equal volume the one with the SMALLEST
 *               root index is the largest (one 64-bit maximum over area << 31 | (2^31 - 1 - root)).  counts[3 C + 1] as above.
 *   Match: min_vox a host scalar >= 0; counts[C][4] int64 = (n_gt, n_gt_hit, n_pred, n_pred_hit), the hit criterion unchanged.
 * Labelling runs the tile and tile-border launches per slice with the in-plane part of the connectivity (4 for 6, 8 for 18 and 26) on
 * volume-wide indices, then one launch in which every voxel with z >= 1 unites with its same-class neighbours in slice z - 1 (agent-scope
 * atomics throughout; one union per run where the voxel directly above matches, the in-plane unions imply the rest), then the flatten
 * launch over the whole volume.  No loop waits for another wave; integer work only: equal inputs give equal bits.
 *
 * dinox_cc3d_ws_bytes: bytes of workspace for any of the three calls, 8 Z H W + 8 C (0 for sizes the calls refuse; contents need not be
 *   initialised; 8-byte aligned).
 * dinox_cc3d_label: connectivity 6, 18 or 26; bad[1] int64, zeroed on the stream first.
 * dinox_cc3d_filter: comp / area as dinox_cc3d_label wrote them for `labels` (same mask, same connectivity).
 * dinox_cc3d_match: pred_comp / pred_area from dinox_cc3d_label(pred, mask = gt), gt_comp / gt_area from dinox_cc3d_label(gt, mask = NULL).
 * ------------------------------------------------------------------------------------------ */
int64_t dinox_cc3d_ws_bytes(int64_t Z, int H, int W, int C);
int dinox_cc3d_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t Z,
                     int H, int W, int C, int connectivity, void* stream);
int dinox_cc3d_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, int min_vox, const uint8_t* y, uint8_t* out,
                      int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int c0, int keep_largest, void* stream);
int dinox_cc3d_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                     const int32_t* gt_area, int min_vox, int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int t_num, int t_den,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Per-launch timing of dinox_gemm (diagnostic; bench.py's roofline object).  Between start and stop every dinox_gemm launch -- also
 * the ones dinox_block_* issue -- is counted per (kernel, shape, epilogue), and one launch in `every` (a fixed hash of the launch
 * counter) is bracketed by a HIP event pair on its stream.  stop synchronises those events and writes one text line per shape into
 * buf:  "<kernel> M N K batch epilogue in_dtype out_dtype has_aux shared_b launches timed ms_timed\n"  and returns the bytes written
 * (-1: buffer too small).  Not for use under graph capture; one timer per process.
 * ------------------------------------------------------------------------------------------ */
int dinox_gemm_timer_start(int every);
int64_t dinox_gemm_timer_stop(char* buf, int64_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* DINOX_H */
