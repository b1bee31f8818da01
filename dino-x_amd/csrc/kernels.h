// kernels.h -- host functions that one .hip file defines and another calls, the bf16 GEMM variant table and the launch glue the
// GEMM launchers share.  Definer and callers include this file, so a changed parameter list is a compile error on both sides.
// A function with no caller outside its own file is not declared here: an extern "C" entry point is defined in the file of its
// kernels, with its argument checks and its launches, and include/dinox.h is its declaration.
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

// ---------------------------------------------------------------- a limit that several kernel families check
constexpr int SEG_MAX_CLASSES = 64;        // segloss.hip: the C logits of a pixel, its softmax and two C-wide accumulators live in a lane's registers;
                                           // surfdist.hip, cclabel.hip and cclabel3d.hip read the same label maps and take the same classes

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
