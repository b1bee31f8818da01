// kernels.h -- host functions that one .hip file defines and another calls, the bf16 GEMM variant table and the launch glue the
// GEMM launchers share.  Definer and callers include this file, so a changed parameter list is a compile error on both sides.
// (Error plumbing, reserve_lds and device_cu_count are in common.h: every file uses those.)
#pragma once
#include <type_traits>

#include "gemm_common.h"
#include "knobs.h"

namespace dinox {

// ---------------------------------------------------------------- bf16 GEMM: which kernel family takes a product
// Member and the name dinox_gemm_kernel_name reports for it (the launch timer keys on it; ops.GemmTimer and tests/test_abi.py compare
// these strings).  None, value 0, has no name: gemm_variant_name gives nullptr.
#define GEMM_VARIANTS(X)                                                                                                       \
  X(NtPp, "gemm_bf16_nt_pp") X(NtPp128, "gemm_bf16_nt_pp128") X(NtPp384, "gemm_bf16_nt_pp384") X(NtAreg, "gemm_bf16_nt_areg") \
  X(NtGlds, "gemm_bf16_nt_glds") X(Nt, "gemm_bf16_nt") X(TnBig, "gemm_bf16_tn_big") X(TnDma, "gemm_bf16_tn_dma") X(Tn, "gemm_bf16_tn")
#define X(member, name) member,
enum class GemmVariant { None, GEMM_VARIANTS(X) };
#undef X
#define X(member, name) name,
inline const char* gemm_variant_name(GemmVariant v) {
  static const char* const names[] = {nullptr, GEMM_VARIANTS(X)};
  return names[(int)v];
}
#undef X

// gemm_f32.hip
int launch_gemm_f32(const GemmParams& p, hipStream_t st);
// gemm_bf16.hip
GemmVariant gemm_bf16_variant(const GemmParams& p);         // family the bf16 dispatcher would use (None: outside all of them)
int launch_gemm_bf16(const GemmParams& p, hipStream_t st);  // returns DINOX_EUNSUPPORTED when it cannot take the shape
int64_t gemm_bf16_ws_bytes(const GemmParams& p);            // workspace of the deterministic split-K reduction (0: none)
// gemm_bf16_glds.hip, gemm_bf16_areg.hip, gemm_bf16_pp.hip, gemm_bf16_pp128.hip, gemm_bf16_pp384.hip: envelope and launcher
bool gemm_bf16_nt_glds_ok(const GemmParams& p);
int launch_gemm_bf16_nt_glds(const GemmParams& p, hipStream_t st);
bool gemm_bf16_nt_areg_ok(const GemmParams& p);
int launch_gemm_bf16_nt_areg(const GemmParams& p, hipStream_t st);
bool gemm_bf16_nt_pp_ok(const GemmParams& p);
int launch_gemm_bf16_nt_pp(const GemmParams& p, hipStream_t st);
bool gemm_bf16_nt_pp128_ok(const GemmParams& p);
int launch_gemm_bf16_nt_pp128(const GemmParams& p, hipStream_t st);
bool gemm_bf16_nt_pp384_ok(const GemmParams& p);
int launch_gemm_bf16_nt_pp384(const GemmParams& p, hipStream_t st);
// gemm_bf16_pp384.hip: the product + LayerNorm form (caller: gemm_bf16_rowln.hip) and the product + LayerNorm-backward form
// (caller: layernorm.hip; ws: pp384_lnbwd_tiles(M) x 2 x 384 floats)
bool gemm_bf16_nt_pp384_ln_ok(int64_t M, int K);
int launch_gemm_bf16_nt_pp384_ln(const void* a, const void* w, const float* bias, const float* residual, float* x_out, const float* gamma,
                                 const float* beta, float eps, void* y, float* mean, float* rstd, int64_t M, int K, hipStream_t st);
int pp384_lnbwd_tiles(int64_t M);
int launch_gemm_bf16_nt_pp384_lnbwd(const void* a, const void* w, const float* x, const float* gamma, const float* mean, const float* rstd,
                                    float* dx, const float* dx_add, void* dx_lowp, float* ws, int64_t M, int K, hipStream_t st);
// gemm_bf16_rowln.hip: does dinox_linear_residual_ln run this width-384 product + LayerNorm (y in y_dtype) on the full-row kernel's
// LayerNorm epilogue instead of its own 128 x 384 kernel?  (callers: dinox_linear_residual_ln's launch choice, dinox_block_plan)
bool linear_residual_ln_full_row(int64_t M, int K, int y_dtype);
// gemm_bf16_tnbig.hip
int tn_big_plan(const GemmParams& p, int& tiles_m, int& tiles_n, int& splits, int64_t& kps);
int64_t tn_big_ws_bytes(const GemmParams& p);
int launch_gemm_bf16_tn_big(const GemmParams& p, hipStream_t st, int& splits_out, int& tiles_n_out);

// ---------------------------------------------------------------- attention (dispatch: attention.hip)
// attention_ref.hip: fp32 math, any dtype
int launch_attention_ref_fwd(const void* qkv, void* o, float* lse, int B, int N, int heads, int d, int dtype, hipStream_t st);
int launch_attention_ref_bwd(const void* d_o, const void* qkv, const void* o, const float* lse, void* dqkv, int B, int N, int heads, int d, int dtype, hipStream_t st);
// attention_bf16.hip: head size 64, whole score strips in registers; DINOX_EUNSUPPORTED outside the envelope
int launch_attention_bf16_fwd(const void* qkv, void* o, float* lse, int B, int N, int heads, int d, hipStream_t st);
int launch_attention_bf16_bwd(const void* d_o, const void* qkv, const void* o, const float* lse, void* dqkv, float* ws, int B, int N, int heads, int d, hipStream_t st);
bool attention_qkv_fused_ok(int B, int N, int heads, int d, int D);
int launch_attention_qkv_fused_fwd(const void* x, const void* w, const float* bias, void* o, void* qkv_out, float* lse, int B, int N, int heads, int d, int D, hipStream_t st);
// attention_flash.hip: any N, d <= 128 (d % 8 == 0)
int launch_attention_flash_fwd(const void* qkv, void* o, float* lse, int B, int N, int heads, int d, hipStream_t st);
int launch_attention_flash_bwd(const void* d_o, const void* qkv, const void* o, const float* lse, void* dqkv, float* ws, int B, int N, int heads, int d, hipStream_t st);

// ---------------------------------------------------------------- NT-Xent (ntxent.hip; entry points and argument checks: abi.hip)
int launch_ntxent_rows(const float* S, int64_t lds, int M, float inv_tau, float* lse, float* row_loss, float* loss, hipStream_t st);
int launch_ntxent_coeff(const float* S, int64_t lds, const float* lse, int M, float inv_tau, float gscale, float* W, int64_t ldw, hipStream_t st);
int launch_ntxent_rows_rect(const float* S, int64_t lds, int Ml, int Mg, int row0, int Bl, float inv_tau, float* lse, float* row_loss,
                            float* loss_sum, hipStream_t st);
int launch_ntxent_coeff_rect(const float* S, int64_t lds, const float* lse_local, const float* lse_all, int Ml, int Mg, int row0, int Bl,
                             float inv_tau, float gscale, float* W, int64_t ldw, hipStream_t st);
int launch_normalize_bwd(const float* dxh, const float* xh, const float* norm, float* dx, int64_t V, int D, float eps, hipStream_t st);

// ---------------------------------------------------------------- attention rows (attention_rows.hip; entry points: abi.hip)
bool attention_rows_ok(int B, int N, int heads, int d, int Q);
int launch_attention_rows(const void* qkv, const int* query_idx, float* probs, float* lse, int B, int N, int heads, int d, int Q, int dtype,
                          hipStream_t st);

// ---------------------------------------------------------------- attention rollout step (attention_rollout.hip; entry points: abi.hip)
bool attention_rollout_step_ok(int B, int N, int heads, int d);
size_t attention_rollout_step_ws_bytes(int B, int N, int heads);
int launch_attention_rollout_step(const void* qkv, const float* w_in, float* w_out, void* ws, int B, int N, int heads, int d, float residual,
                                  int dtype, hipStream_t st);

// ---------------------------------------------------------------- MAE masked-token glue (mae.hip; entry points and argument checks: abi.hip)
constexpr int MAE_MAX_L = 4096;      // patches per sample: the sort keys of one sample sit in LDS
constexpr int MAE_MAX_PATCH = 32;    // patch edge of the loss kernels: one target patch (3 p^2 floats) sits in LDS
int launch_mae_mask_ids(const float* noise, int* ids_restore, int* ids_keep, int V, int L, int Lk, hipStream_t st);
int launch_mae_gather_unfold(const float* x, const int* ids_keep, void* u, int V, int H, int W, int patch, int Lk, int ld, int dtype,
                             hipStream_t st);
int launch_mae_tokens_fwd(const void* patches, const float* cls, const float* pos, const int* ids_keep, float* tok, int V, int L, int Lk,
                          int D, int dtype, hipStream_t st);
int launch_mae_tokens_bwd(const float* dtok, const int* ids_restore, void* dpatches, float* dcls, float* dpos, int V, int L, int Lk, int D,
                          int dtype, hipStream_t st);
int launch_mae_unshuffle_fwd(const void* e, const float* mask_token, const float* dpe, const int* ids_restore, float* xd, int V, int L,
                             int Lk, int D, int dtype, hipStream_t st);
int launch_mae_unshuffle_bwd(const float* g, const int* ids_keep, const int* ids_restore, void* de, float* dmask, float* ws, int V, int L,
                             int Lk, int D, int dtype, hipStream_t st);
int launch_mae_loss_fwd(const void* pred, const float* x, const int* ids_restore, float* loss, float* ws, int V, int H, int W, int patch,
                        int Lk, int lead, int dtype, hipStream_t st);
int launch_mae_loss_bwd(const void* pred, const float* x, const int* ids_restore, void* dpred, float gscale, int V, int H, int W, int patch,
                        int Lk, int lead, int dtype, int out_dtype, hipStream_t st);

// ---------------------------------------------------------------- iBOT masked-patch objective (ibot.hip; entry points and argument checks: abi.hip)
constexpr int IBOT_MASK_CHUNK = 64;        // masked rows per partial sum of put_mask_bwd: ws holds ceil(M / 64) x D floats
constexpr int IBOT_CE_REG_MAX_K = 8192;    // widest row the register-resident cross-entropy holds: 8 float4 per thread and matrix
int launch_ibot_put_mask(void* patches, const float* mask_token, const int* idx, int M, int64_t rows, int D, int dtype, hipStream_t st);
int launch_ibot_put_mask_bwd(void* dpatches, const int* idx, float* dmask, float* ws, int M, int64_t rows, int D, int dtype, hipStream_t st);
int launch_gather_rows(const float* src, const int* row, void* dst, int64_t M, int64_t src_rows, int D, int64_t dst_row0, int dtype,
                       hipStream_t st);
int launch_scatter_add_rows(const void* src, const int* row, float* dst, int64_t M, int64_t dst_rows, int D, int64_t src_row0, int dtype,
                            hipStream_t st);
int launch_ibot_ce(const float* s, const float* t, const float* center, const float* w, float inv_ts, float inv_tt, float scale, float gscale,
                   float* loss, float* ds, float* row_loss, int M, int K, hipStream_t st);
int launch_ibot_center_ema(float* center, const float* sum_count, float momentum, int K, hipStream_t st);

// ---------------------------------------------------------------- LoRA low-rank products (lora.hip; entry points and argument checks: abi.hip)
constexpr int LORA_MAX_RANK = 64;          // two 32-wide accumulator blocks per wave; u and v of one row chunk (2 x 128 x r floats) sit in LDS beside a 66 KiB tile
constexpr int LORA_GRAD_CHUNK = 128;       // rows per partial sum of dinox_lora_grad: ws holds ceil(M / 128) x (r K + N r) floats
int launch_lora_down(const void* x, const float* S, float* u, int64_t M, int Kd, int r, int layout, int dtype, hipStream_t st);
bool lora_up_grid_ok(int64_t M, int N);
int launch_lora_up(const float* u, const float* S, const float* res, float* t, float s, int64_t M, int N, int r, int layout, hipStream_t st);
int64_t lora_grad_chunks(int64_t M);
int launch_lora_grad(const void* xl, const void* dy, const float* A, const float* B, float s, float* dA, float* dB, float* ws, int64_t M, int K,
                     int N, int r, int dtype, hipStream_t st);
int launch_lora_dropout(const void* in, void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, hipStream_t st);

// ---------------------------------------------------------------- dense segmentation loss (segloss.hip; entry points and argument checks: abi.hip)
constexpr int SEG_MAX_CLASSES = 64;        // the C logits of a pixel, its softmax and two C-wide accumulators live in a lane's registers
constexpr int SEG_MAX_UPSAMPLE = 32;       // a cell (the pixels that share their four taps) is at most 1.5 u = 48 columns: one wave row
constexpr int SEG_FWD_CELLS = 8;           // cells per partial sum of dinox_seg_loss_fwd
int64_t seg_loss_ws_bytes(int64_t B, int g, int C);
int launch_seg_loss_fwd(const float* z, const uint8_t* y, float* loss, float* stats, int64_t* nv, void* ws, int64_t B, int g, int u, int C, int c0,
                        float w_ce, float w_dice, hipStream_t st);
int launch_seg_loss_bwd(const float* z, const uint8_t* y, const float* stats, const int64_t* nv, float* dz, void* ws, int64_t B, int g, int u, int C,
                        int c0, float w_ce, float w_dice, float gscale, hipStream_t st);
int launch_seg_predict(const float* z, const uint8_t* y, uint8_t* pred, int64_t* counts, int64_t B, int g, int u, int C, hipStream_t st);

// ---------------------------------------------------------------- surface distances of two label maps (surfdist.hip; entry point and argument checks: abi.hip)
constexpr int SURF_MAX_SIDE = 1024;        // a row of squared column distances (4 KiB) sits in LDS; a column distance fits uint16 beside its sentinel
constexpr int SURF_MAX_TOL = 8;            // tolerance counters per lane, in registers
int64_t surface_ws_bytes(int64_t B, int H, int W, int C);
int launch_surface_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values, int64_t* bad,
                         void* ws, int64_t B, int H, int W, int C, int T, int q_num, int q_den, hipStream_t st);

// ---------------------------------------------------------------- connected components of a label map (cclabel.hip; entry points and argument checks: abi.hip)
constexpr int CC_MAX_SIDE = 1024;          // a root index y W + x and an area both fit 20 bits beside each other in the 64-bit tie key
int64_t cc_ws_bytes(int64_t B, int H, int W, int C);
int launch_cc_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t B, int H,
                    int W, int C, int conn, hipStream_t st);
int launch_cc_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, const uint8_t* y, uint8_t* out,
                     int64_t* counts, void* ws, int64_t B, int H, int W, int C, int c0, int keep_largest, hipStream_t st);
int launch_cc_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                    const int32_t* gt_area, const int32_t* min_px, int64_t* counts, void* ws, int64_t B, int H, int W, int C, int t_num, int t_den,
                    hipStream_t st);

// ---------------------------------------------------------------- connected components of one label volume (cclabel3d.hip on cclabel.hip's stages; abi.hip)
constexpr int64_t CC3D_MAX_VOXELS = (int64_t)1 << 30;   // every voxel index and every area fits int32, and 31 bits of the 64-bit tie key
int64_t cc3d_ws_bytes(int64_t Z, int H, int W, int C);
int launch_cc3d_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t Z, int H,
                      int W, int C, int conn, hipStream_t st);
int launch_cc3d_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, int min_vox, const uint8_t* y, uint8_t* out, int64_t* counts,
                       void* ws, int64_t Z, int H, int W, int C, int c0, int keep_largest, hipStream_t st);
int launch_cc3d_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                      const int32_t* gt_area, int min_vox, int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int t_num, int t_den, hipStream_t st);

// ---------------------------------------------------------------- launch glue shared by the NT launchers
// Activation index of the <OUT, ACT, RES> kernels (gemm_bf16_pp / _pp128 / _areg): the template argument ACT.
enum { EPI_ACT_PLAIN = 0, EPI_ACT_GELU = 1, EPI_ACT_DGELU = 2 };

// (out_dtype, epilogue) -> f(OUT, ACT, RES) with the three as std::integral_constant values (decltype(x)::value is the template
// argument); returns what f returns.  The kernels are built for four cases -- plain, plain + residual, GELU, GELU' -- and every
// other combination is DINOX_EUNSUPPORTED.
template <typename F>
static inline int with_epilogue_case(const GemmParams& p, F&& f) {
  const int act = (p.epilogue & DINOX_EPI_GELU) ? EPI_ACT_GELU : (p.epilogue & DINOX_EPI_DGELU) ? EPI_ACT_DGELU : EPI_ACT_PLAIN;
  const bool res = (p.epilogue & DINOX_EPI_RESIDUAL) != 0;
  auto cases = [&](auto out) -> int {
    switch (act * 2 + (res ? 1 : 0)) {
      case 0: return f(out, std::integral_constant<int, EPI_ACT_PLAIN>{}, std::false_type{});
      case 1: return f(out, std::integral_constant<int, EPI_ACT_PLAIN>{}, std::true_type{});
      case 2: return f(out, std::integral_constant<int, EPI_ACT_GELU>{}, std::false_type{});
      case 4: return f(out, std::integral_constant<int, EPI_ACT_DGELU>{}, std::false_type{});
      default: return DINOX_EUNSUPPORTED;
    }
  };
  return p.out_dtype == DINOX_BF16 ? cases(std::integral_constant<int, DINOX_BF16>{}) : cases(std::integral_constant<int, DINOX_F32>{});
}

// Launch plan of a persistent kernel on BM x BN tiles: one workgroup per CU walks `units` tiles in `order` (DINOX_PP_ORDER) after a
// start delay of `stagger` cycles.  The kernel's own stagger rule comes in as stagger_auto; DINOX_PP_STAGGER overrides it.
struct PersistPlan {
  int tiles_n, units, order, stagger;
  unsigned grid;
};
static inline bool persist_plan(const GemmParams& p, int bm, int bn, int stagger_auto, PersistPlan& pl) {
  const int64_t tiles_n = ceil_div(p.N, (int64_t)bn), units = ceil_div(p.M, (int64_t)bm) * tiles_n;
  if (units > 0x3fffffff) return false;
  const int64_t ncu = device_cu_count();
  pl = {(int)tiles_n, (int)units, knob_int("DINOX_PP_ORDER", 1), knob_int("DINOX_PP_STAGGER", stagger_auto), (unsigned)(units < ncu ? units : ncu)};
  return true;
}

}  // namespace dinox
