// abi.hip -- error plumbing and library-level entry points of libdinox_hip.so.
#include <cstdarg>
#include <cstring>
#include <mutex>
#include <unordered_map>

#include "common.h"
#include "kernels.h"

namespace dinox {

static thread_local char g_err[512] = {0};

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// Raise a kernel's dynamic-LDS limit, ONCE per (kernel, size).  hipFuncSetAttribute is not a stream operation and must not be
// issued while a stream is being captured into a hipGraph; after the first eager launch of a shape it is never called again, so
// a captured step (dinox.engine.TrainEngine(use_graph=True)) holds kernel nodes only.
int reserve_lds(const void* kern, size_t bytes, const char* what) {
  if (bytes <= 64 * 1024) return 0;
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> granted;
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = granted[kern];
  if (bytes <= have) return 0;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail((int)e, "%s: cannot reserve %zu B of LDS (%s)", what, bytes, hipGetErrorString(e));
  }
  have = bytes;
  return 0;
}

int device_cu_count() {
  static const int ncu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) (void)hipGetLastError();
    return n > 0 ? n : 256;
  }();
  return ncu;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace dinox

extern "C" int dinox_version(void) { return DINOX_ABI_VERSION; }

extern "C" const char* dinox_last_error(void) { return dinox::g_err; }

extern "C" int dinox_device_ok(void) {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    dinox::set_error("no HIP device visible (hipGetDeviceCount: %s, %d devices)", hipGetErrorString(e), n);
    return 0;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) {
    (void)hipGetLastError();
    dinox::set_error("hipGetDeviceProperties failed");
    return 0;
  }
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    dinox::set_error("device 0 is %s, this library is built for gfx950 only", prop.gcnArchName);
    return 0;
  }
  return 1;
}

// ---------------------------------------------------------------- NT-Xent entry points (kernels: ntxent.hip)
static bool ntxent_rows_ok(int M) { return M >= 2 && M % 2 == 0 && M <= 65535 * 32; }

extern "C" int dinox_ntxent_rows(const float* S, int64_t lds, int M, float inv_tau, float* lse, float* row_loss, float* loss, void* stream) {
  DX_REQUIRE(S && lse && row_loss && loss, DINOX_EINVAL, "ntxent_rows: null pointer");
  DX_REQUIRE(ntxent_rows_ok(M), DINOX_EINVAL, "ntxent_rows: M=%d (the rows are [z1; z2]: an even count of at least 2)", M);
  DX_REQUIRE(lds >= M && inv_tau > 0.f, DINOX_EINVAL, "ntxent_rows: lds=%lld M=%d inv_tau=%g", (long long)lds, M, (double)inv_tau);
  return dinox::launch_ntxent_rows(S, lds, M, inv_tau, lse, row_loss, loss, dinox::as_stream(stream));
}

extern "C" int dinox_ntxent_coeff(const float* S, int64_t lds, const float* lse, int M, float inv_tau, float gscale, float* W, int64_t ldw,
                                  void* stream) {
  DX_REQUIRE(S && lse && W, DINOX_EINVAL, "ntxent_coeff: null pointer");
  DX_REQUIRE(ntxent_rows_ok(M), DINOX_EINVAL, "ntxent_coeff: M=%d (the rows are [z1; z2]: an even count of at least 2)", M);
  DX_REQUIRE(lds >= M && ldw >= M && inv_tau > 0.f, DINOX_EINVAL, "ntxent_coeff: lds=%lld ldw=%lld M=%d inv_tau=%g", (long long)lds,
             (long long)ldw, M, (double)inv_tau);
  DX_REQUIRE(W != S, DINOX_EINVAL, "ntxent_coeff: W must not alias S (a tile reads its mirror image, which another workgroup writes)");
  return dinox::launch_ntxent_coeff(S, lds, lse, M, inv_tau, gscale, W, ldw, dinox::as_stream(stream));
}

// The rectangular forms: Ml = 2 Bl local rows against Mg = world * Ml gathered columns, this rank's block at column row0.
static int ntxent_rect_ok(const char* what, int64_t lds, int Ml, int Mg, int row0, int Bl, float inv_tau) {
  DX_REQUIRE(ntxent_rows_ok(Ml), DINOX_EINVAL, "%s: Ml=%d (the local rows are [z1; z2]: an even count of at least 2)", what, Ml);
  DX_REQUIRE(Bl * 2 == Ml, DINOX_EINVAL, "%s: Bl=%d is not half of Ml=%d", what, Bl, Ml);
  DX_REQUIRE(Mg >= Ml && Mg % Ml == 0 && Mg <= 65535 * 32, DINOX_EINVAL, "%s: Mg=%d is not a multiple of Ml=%d (every rank holds Ml rows)", what,
             Mg, Ml);
  DX_REQUIRE(row0 >= 0 && row0 <= Mg - Ml && row0 % Ml == 0, DINOX_EINVAL, "%s: row0=%d is not the start of a rank's block (Ml=%d, Mg=%d)", what,
             row0, Ml, Mg);
  DX_REQUIRE(lds >= Mg && inv_tau > 0.f, DINOX_EINVAL, "%s: lds=%lld Mg=%d inv_tau=%g", what, (long long)lds, Mg, (double)inv_tau);
  return 0;
}

extern "C" int dinox_ntxent_rows_rect(const float* S, int64_t lds, int Ml, int Mg, int row0, int Bl, float inv_tau, float* lse, float* row_loss,
                                      float* loss_sum, void* stream) {
  DX_REQUIRE(S && lse && row_loss && loss_sum, DINOX_EINVAL, "ntxent_rows_rect: null pointer");
  const int rc = ntxent_rect_ok("ntxent_rows_rect", lds, Ml, Mg, row0, Bl, inv_tau);
  if (rc) return rc;
  return dinox::launch_ntxent_rows_rect(S, lds, Ml, Mg, row0, Bl, inv_tau, lse, row_loss, loss_sum, dinox::as_stream(stream));
}

extern "C" int dinox_ntxent_coeff_rect(const float* S, int64_t lds, const float* lse_local, const float* lse_all, int Ml, int Mg, int row0,
                                       int Bl, float inv_tau, float gscale, float* W, int64_t ldw, void* stream) {
  DX_REQUIRE(S && lse_local && lse_all && W, DINOX_EINVAL, "ntxent_coeff_rect: null pointer");
  const int rc = ntxent_rect_ok("ntxent_coeff_rect", lds, Ml, Mg, row0, Bl, inv_tau);
  if (rc) return rc;
  DX_REQUIRE(ldw >= Mg, DINOX_EINVAL, "ntxent_coeff_rect: ldw=%lld Mg=%d", (long long)ldw, Mg);
  return dinox::launch_ntxent_coeff_rect(S, lds, lse_local, lse_all, Ml, Mg, row0, Bl, inv_tau, gscale, W, ldw, dinox::as_stream(stream));
}

extern "C" int dinox_normalize_bwd(const float* dxh, const float* xh, const float* norm, float* dx, int64_t V, int D, float eps, void* stream) {
  DX_REQUIRE(dxh && xh && norm && dx, DINOX_EINVAL, "normalize_bwd: null pointer");
  DX_REQUIRE(V > 0 && V <= 0x7fffffff && D > 0 && eps > 0.f, DINOX_EINVAL, "normalize_bwd: V=%lld D=%d eps=%g", (long long)V, D, (double)eps);
  return dinox::launch_normalize_bwd(dxh, xh, norm, dx, V, D, eps, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- attention rows (kernel: attention_rows.hip)
extern "C" int dinox_attention_rows_ok(int B, int N, int heads, int d, int Q) { return dinox::attention_rows_ok(B, N, heads, d, Q) ? 1 : 0; }

extern "C" int dinox_attention_rows(const void* qkv, const int* query_idx, float* probs, float* lse, int B, int N, int heads, int d, int Q,
                                    int dtype, void* stream) {
  DX_REQUIRE(qkv && query_idx && probs, DINOX_EINVAL, "attention_rows: null pointer");
  DX_REQUIRE(dtype == DINOX_F32 || dtype == DINOX_BF16, DINOX_EINVAL, "attention_rows: dtype %d", dtype);
  DX_REQUIRE(dinox::attention_rows_ok(B, N, heads, d, Q), DINOX_EINVAL,
             "attention_rows: B=%d N=%d heads=%d d=%d Q=%d (B, N, heads >= 1; 1 <= d <= 256; 1 <= Q <= 8)", B, N, heads, d, Q);
  return dinox::launch_attention_rows(qkv, query_idx, probs, lse, B, N, heads, d, Q, dtype, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- attention rollout step (kernels: attention_rollout.hip)
extern "C" int dinox_attention_rollout_step_ok(int B, int N, int heads, int d) { return dinox::attention_rollout_step_ok(B, N, heads, d) ? 1 : 0; }

extern "C" size_t dinox_attention_rollout_step_ws_bytes(int B, int N, int heads) { return dinox::attention_rollout_step_ws_bytes(B, N, heads); }

extern "C" int dinox_attention_rollout_step(const void* qkv, const float* w_in, float* w_out, void* ws, int B, int N, int heads, int d,
                                            float residual, int dtype, void* stream) {
  DX_REQUIRE(qkv && w_in && w_out && ws, DINOX_EINVAL, "attention_rollout_step: null pointer");
  DX_REQUIRE(dtype == DINOX_F32 || dtype == DINOX_BF16, DINOX_EINVAL, "attention_rollout_step: dtype %d", dtype);
  DX_REQUIRE(dinox::attention_rollout_step_ok(B, N, heads, d), DINOX_EINVAL,
             "attention_rollout_step: B=%d N=%d heads=%d d=%d (B, heads >= 1; 1 <= N <= 4096; 1 <= d <= 256)", B, N, heads, d);
  DX_REQUIRE(residual >= 0.f && residual <= 1.f, DINOX_EINVAL, "attention_rollout_step: residual %g outside [0, 1]", (double)residual);
  const float* in_end = w_in + (size_t)B * N;
  const float* out_end = w_out + (size_t)B * N;
  DX_REQUIRE(in_end <= w_out || out_end <= w_in, DINOX_EINVAL, "attention_rollout_step: w_out must not alias w_in (the fold reads w_in)");
  return dinox::launch_attention_rollout_step(qkv, w_in, w_out, ws, B, N, heads, d, residual, dtype, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- MAE masked-token glue (kernels: mae.hip)
static bool mae_dtype_ok(int dt) { return dt == DINOX_F32 || dt == DINOX_BF16; }
// V samples of L patches of which 1 <= Lk < L are kept; D features.  (V * (1 + L) rows index a 32-bit grid in the loss kernels.)
static bool mae_shape_ok(int V, int L, int Lk, int D) {
  return V >= 1 && V <= (1 << 20) && L >= 2 && L <= dinox::MAE_MAX_L && Lk >= 1 && Lk < L && D >= 1 && D <= (1 << 16) &&
         (int64_t)V * (1 + L) <= 0x7fffffff;
}
static bool mae_image_ok(int V, int H, int W, int patch, int Lk) {
  if (!(H > 0 && W > 0 && patch > 0 && H % patch == 0 && W % patch == 0 && H <= (1 << 14) && W <= (1 << 14))) return false;
  const int64_t L = (int64_t)(H / patch) * (W / patch);
  return L <= dinox::MAE_MAX_L && mae_shape_ok(V, (int)L, Lk, 1);
}

extern "C" int dinox_mae_mask_ids(const float* noise, int* ids_restore, int* ids_keep, int V, int L, int Lk, void* stream) {
  DX_REQUIRE(noise && ids_restore && ids_keep, DINOX_EINVAL, "mae_mask_ids: null pointer");
  DX_REQUIRE(mae_shape_ok(V, L, Lk, 1), DINOX_EINVAL, "mae_mask_ids: V=%d L=%d Lk=%d (V >= 1, 2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, dinox::MAE_MAX_L);
  return dinox::launch_mae_mask_ids(noise, ids_restore, ids_keep, V, L, Lk, dinox::as_stream(stream));
}

extern "C" int dinox_mae_gather_unfold(const float* x, const int* ids_keep, void* u, int V, int H, int W, int patch, int Lk, int ld,
                                       int out_dtype, void* stream) {
  DX_REQUIRE(x && ids_keep && u, DINOX_EINVAL, "mae_gather_unfold: null pointer");
  DX_REQUIRE(mae_dtype_ok(out_dtype), DINOX_EINVAL, "mae_gather_unfold: dtype %d", out_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= 1024 && ld >= 3 * patch * patch && ld <= (1 << 22), DINOX_EINVAL,
             "mae_gather_unfold: V=%d H=%d W=%d patch=%d Lk=%d ld=%d (H, W multiples of patch; 2 <= L <= %d; 1 <= Lk < L; ld >= 3 patch^2)", V, H,
             W, patch, Lk, ld, dinox::MAE_MAX_L);
  return dinox::launch_mae_gather_unfold(x, ids_keep, u, V, H, W, patch, Lk, ld, out_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_tokens_fwd(const void* patches, const float* cls, const float* pos, const int* ids_keep, float* tokens, int V, int L,
                                    int Lk, int D, int patches_dtype, void* stream) {
  DX_REQUIRE(patches && cls && pos && ids_keep && tokens, DINOX_EINVAL, "mae_tokens_fwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(patches_dtype), DINOX_EINVAL, "mae_tokens_fwd: dtype %d", patches_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_tokens_fwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, dinox::MAE_MAX_L);
  return dinox::launch_mae_tokens_fwd(patches, cls, pos, ids_keep, tokens, V, L, Lk, D, patches_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_tokens_bwd(const float* dtokens, const int* ids_restore, void* dpatches, float* dcls, float* dpos, int V, int L, int Lk,
                                    int D, int patches_dtype, void* stream) {
  DX_REQUIRE(dtokens && ids_restore && dpatches && dcls && dpos, DINOX_EINVAL, "mae_tokens_bwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(patches_dtype), DINOX_EINVAL, "mae_tokens_bwd: dtype %d", patches_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_tokens_bwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, dinox::MAE_MAX_L);
  return dinox::launch_mae_tokens_bwd(dtokens, ids_restore, dpatches, dcls, dpos, V, L, Lk, D, patches_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_unshuffle_fwd(const void* e, const float* mask_token, const float* dec_pos, const int* ids_restore, float* xd, int V,
                                       int L, int Lk, int D, int e_dtype, void* stream) {
  DX_REQUIRE(e && mask_token && dec_pos && ids_restore && xd, DINOX_EINVAL, "mae_unshuffle_fwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(e_dtype), DINOX_EINVAL, "mae_unshuffle_fwd: dtype %d", e_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_unshuffle_fwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, dinox::MAE_MAX_L);
  return dinox::launch_mae_unshuffle_fwd(e, mask_token, dec_pos, ids_restore, xd, V, L, Lk, D, e_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_unshuffle_bwd(const float* g, const int* ids_keep, const int* ids_restore, void* de, float* dmask_token, float* ws,
                                       int V, int L, int Lk, int D, int de_dtype, void* stream) {
  DX_REQUIRE(g && ids_keep && ids_restore && de && dmask_token && ws, DINOX_EINVAL, "mae_unshuffle_bwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(de_dtype), DINOX_EINVAL, "mae_unshuffle_bwd: dtype %d", de_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_unshuffle_bwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, dinox::MAE_MAX_L);
  return dinox::launch_mae_unshuffle_bwd(g, ids_keep, ids_restore, de, dmask_token, ws, V, L, Lk, D, de_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_loss_fwd(const void* pred, const float* x, const int* ids_restore, float* loss, float* ws, int V, int H, int W, int patch,
                                  int Lk, int lead, int pred_dtype, void* stream) {
  DX_REQUIRE(pred && x && ids_restore && loss && ws, DINOX_EINVAL, "mae_loss_fwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(pred_dtype), DINOX_EINVAL, "mae_loss_fwd: dtype %d", pred_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= dinox::MAE_MAX_PATCH && (lead == 0 || lead == 1), DINOX_EINVAL,
             "mae_loss_fwd: V=%d H=%d W=%d patch=%d Lk=%d lead=%d (H, W multiples of patch <= %d; 2 <= L <= %d; 1 <= Lk < L; lead 0 or 1)", V, H, W,
             patch, Lk, lead, dinox::MAE_MAX_PATCH, dinox::MAE_MAX_L);
  return dinox::launch_mae_loss_fwd(pred, x, ids_restore, loss, ws, V, H, W, patch, Lk, lead, pred_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_mae_loss_bwd(const void* pred, const float* x, const int* ids_restore, void* dpred, float gscale, int V, int H, int W,
                                  int patch, int Lk, int lead, int pred_dtype, int dpred_dtype, void* stream) {
  DX_REQUIRE(pred && x && ids_restore && dpred, DINOX_EINVAL, "mae_loss_bwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(pred_dtype) && mae_dtype_ok(dpred_dtype), DINOX_EINVAL, "mae_loss_bwd: dtypes %d, %d", pred_dtype, dpred_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= dinox::MAE_MAX_PATCH && (lead == 0 || lead == 1), DINOX_EINVAL,
             "mae_loss_bwd: V=%d H=%d W=%d patch=%d Lk=%d lead=%d (H, W multiples of patch <= %d; 2 <= L <= %d; 1 <= Lk < L; lead 0 or 1)", V, H, W,
             patch, Lk, lead, dinox::MAE_MAX_PATCH, dinox::MAE_MAX_L);
  DX_REQUIRE(dpred != pred, DINOX_EINVAL, "mae_loss_bwd: dpred must not alias pred");
  return dinox::launch_mae_loss_bwd(pred, x, ids_restore, dpred, gscale, V, H, W, patch, Lk, lead, pred_dtype, dpred_dtype, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- iBOT masked-patch objective (kernels: ibot.hip)
// M masked rows out of `rows` (flat int32 positions), D features.
static bool ibot_rows_ok(int64_t M, int64_t rows, int D) {
  return M >= 1 && M <= 0x7fffffff && rows >= 1 && rows <= 0x7fffffff && D >= 1 && D <= (1 << 16);
}

extern "C" int dinox_ibot_put_mask(void* patches, const float* mask_token, const int* idx, int M, int64_t rows, int D, int dtype, void* stream) {
  DX_REQUIRE(patches && mask_token && idx, DINOX_EINVAL, "ibot_put_mask: null pointer");
  DX_REQUIRE(mae_dtype_ok(dtype), DINOX_EINVAL, "ibot_put_mask: dtype %d", dtype);
  DX_REQUIRE(ibot_rows_ok(M, rows, D), DINOX_EINVAL, "ibot_put_mask: M=%d rows=%lld D=%d (M, rows >= 1; 1 <= D <= 65536)", M, (long long)rows, D);
  return dinox::launch_ibot_put_mask(patches, mask_token, idx, M, rows, D, dtype, dinox::as_stream(stream));
}

extern "C" int dinox_ibot_put_mask_bwd(void* dpatches, const int* idx, float* dmask_token, float* ws, int M, int64_t rows, int D, int dtype,
                                       void* stream) {
  DX_REQUIRE(dpatches && idx && dmask_token && ws, DINOX_EINVAL, "ibot_put_mask_bwd: null pointer");
  DX_REQUIRE(mae_dtype_ok(dtype), DINOX_EINVAL, "ibot_put_mask_bwd: dtype %d", dtype);
  DX_REQUIRE(ibot_rows_ok(M, rows, D) && M <= 65535 * dinox::IBOT_MASK_CHUNK, DINOX_EINVAL,
             "ibot_put_mask_bwd: M=%d rows=%lld D=%d (1 <= M <= %d; rows >= 1; 1 <= D <= 65536)", M, (long long)rows, D,
             65535 * dinox::IBOT_MASK_CHUNK);
  return dinox::launch_ibot_put_mask_bwd(dpatches, idx, dmask_token, ws, M, rows, D, dtype, dinox::as_stream(stream));
}

extern "C" int dinox_gather_rows(const float* src, const int* row, void* dst, int64_t M, int64_t src_rows, int D, int64_t dst_row0, int dst_dtype,
                                 void* stream) {
  DX_REQUIRE(src && row && dst, DINOX_EINVAL, "gather_rows: null pointer");
  DX_REQUIRE(mae_dtype_ok(dst_dtype), DINOX_EINVAL, "gather_rows: dtype %d", dst_dtype);
  DX_REQUIRE(ibot_rows_ok(M, src_rows, D) && dst_row0 >= 0, DINOX_EINVAL, "gather_rows: M=%lld src_rows=%lld D=%d dst_row0=%lld", (long long)M,
             (long long)src_rows, D, (long long)dst_row0);
  return dinox::launch_gather_rows(src, row, dst, M, src_rows, D, dst_row0, dst_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_scatter_add_rows(const void* src, const int* row, float* dst, int64_t M, int64_t dst_rows, int D, int64_t src_row0,
                                      int src_dtype, void* stream) {
  DX_REQUIRE(src && row && dst, DINOX_EINVAL, "scatter_add_rows: null pointer");
  DX_REQUIRE(mae_dtype_ok(src_dtype), DINOX_EINVAL, "scatter_add_rows: dtype %d", src_dtype);
  DX_REQUIRE(ibot_rows_ok(M, dst_rows, D) && src_row0 >= 0, DINOX_EINVAL, "scatter_add_rows: M=%lld dst_rows=%lld D=%d src_row0=%lld", (long long)M,
             (long long)dst_rows, D, (long long)src_row0);
  return dinox::launch_scatter_add_rows(src, row, dst, M, dst_rows, D, src_row0, src_dtype, dinox::as_stream(stream));
}

extern "C" int dinox_ibot_ce(const float* s, const float* t, const float* center, const float* w, float student_temp, float teacher_temp,
                             float scale, float grad_scale, float* loss, float* ds, float* row_loss, int M, int K, void* stream) {
  DX_REQUIRE(s && t && center && w && loss && row_loss, DINOX_EINVAL, "ibot_ce: null pointer");
  DX_REQUIRE(M >= 1 && K >= 1, DINOX_EINVAL, "ibot_ce: M=%d K=%d", M, K);
  DX_REQUIRE(student_temp > 0.f && teacher_temp > 0.f, DINOX_EINVAL, "ibot_ce: temperatures must be > 0");
  if (ds) {
    const size_t n = (size_t)M * (size_t)K;
    const float* de = ds + n;
    DX_REQUIRE((de <= s || s + n <= ds) && (de <= t || t + n <= ds), DINOX_EINVAL, "ibot_ce: ds must not alias s or t");
  }
  return dinox::launch_ibot_ce(s, t, center, w, 1.0f / student_temp, 1.0f / teacher_temp, scale, grad_scale * scale, loss, ds, row_loss, M, K,
                               dinox::as_stream(stream));
}

extern "C" int dinox_ibot_center_ema(float* center, const float* sum_count, float momentum, int K, void* stream) {
  DX_REQUIRE(center && sum_count && K >= 1, DINOX_EINVAL, "ibot_center_ema: bad arguments");
  return dinox::launch_ibot_center_ema(center, sum_count, momentum, K, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- dense segmentation loss (kernels: segloss.hip)
// 0, or the error code after the message is set.  B g^2 cells and B S^2 pixels stay far inside int64 and the grids inside 2^31 - 1.
static int seg_geometry(const char* who, int64_t B, int g, int u, int C) {
  DX_REQUIRE(B >= 1 && B <= (1 << 20) && g >= 1 && g <= 4096, DINOX_EINVAL, "%s: B=%lld g=%d (1 <= B <= 2^20; 1 <= g <= 4096)", who, (long long)B, g);
  DX_REQUIRE(u >= 1 && u <= dinox::SEG_MAX_UPSAMPLE, DINOX_EINVAL, "%s: u=%d (1 <= u <= %d)", who, u, dinox::SEG_MAX_UPSAMPLE);
  DX_REQUIRE(C >= 2, DINOX_EINVAL, "%s: C=%d (2 <= C <= %d)", who, C, dinox::SEG_MAX_CLASSES);
  DX_REQUIRE(C <= dinox::SEG_MAX_CLASSES, DINOX_EUNSUPPORTED, "%s: C=%d classes: at most %d are held in registers", who, C, dinox::SEG_MAX_CLASSES);
  DX_REQUIRE(B * g * g <= ((int64_t)1 << 32), DINOX_EINVAL, "%s: B g^2 = %lld cells (at most 2^32)", who, (long long)(B * g * g));
  return 0;
}

extern "C" int64_t dinox_seg_loss_ws_bytes(int64_t B, int g, int u, int C) {
  if (B < 1 || B > (1 << 20) || g < 1 || g > 4096 || u < 1 || u > dinox::SEG_MAX_UPSAMPLE || C < 2 || C > dinox::SEG_MAX_CLASSES ||
      B * g * g > ((int64_t)1 << 32))
    return 0;
  return dinox::seg_loss_ws_bytes(B, g, C);
}

extern "C" int dinox_seg_loss_fwd(const float* z, const uint8_t* y, float* loss, float* stats, int64_t* nv, void* ws, int64_t B, int g, int u, int C,
                                  int c0, float w_ce, float w_dice, void* stream) {
  DX_REQUIRE(z && y && loss && stats && nv && ws, DINOX_EINVAL, "seg_loss_fwd: null pointer");
  const int rc = seg_geometry("seg_loss_fwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_fwd: c0=%d (0: every class in the Dice term, 1: without class 0)", c0);
  return dinox::launch_seg_loss_fwd(z, y, loss, stats, nv, ws, B, g, u, C, c0, w_ce, w_dice, dinox::as_stream(stream));
}

extern "C" int dinox_seg_loss_bwd(const float* z, const uint8_t* y, const float* stats, const int64_t* nv, float* dz, void* ws, int64_t B, int g,
                                  int u, int C, int c0, float w_ce, float w_dice, float grad_scale, void* stream) {
  DX_REQUIRE(z && y && stats && nv && dz && ws, DINOX_EINVAL, "seg_loss_bwd: null pointer");
  const int rc = seg_geometry("seg_loss_bwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_bwd: c0=%d (0: every class in the Dice term, 1: without class 0)", c0);
  return dinox::launch_seg_loss_bwd(z, y, stats, nv, dz, ws, B, g, u, C, c0, w_ce, w_dice, grad_scale, dinox::as_stream(stream));
}

extern "C" int dinox_seg_predict(const float* z, const uint8_t* y, uint8_t* pred, int64_t* counts, int64_t B, int g, int u, int C, void* stream) {
  DX_REQUIRE(z && pred, DINOX_EINVAL, "seg_predict: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "seg_predict: labels and counts come together (both or neither)");
  const int rc = seg_geometry("seg_predict", B, g, u, C);
  if (rc) return rc;
  return dinox::launch_seg_predict(z, y, pred, counts, B, g, u, C, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- surface distances of two label maps (kernels: surfdist.hip)
// B C 2 H workgroups (the row launch) stay inside 2^30 and every plane index inside int64.
static bool surface_sizes_ok(int64_t B, int H, int W, int C) {
  return B >= 1 && B <= (1 << 20) && H >= 1 && H <= dinox::SURF_MAX_SIDE && W >= 1 && W <= dinox::SURF_MAX_SIDE && C >= 2 && C <= dinox::SEG_MAX_CLASSES &&
         B * C * 2 * H <= ((int64_t)1 << 30);
}

extern "C" int64_t dinox_surface_ws_bytes(int64_t B, int H, int W, int C) {
  return surface_sizes_ok(B, H, W, C) ? dinox::surface_ws_bytes(B, H, W, C) : 0;
}

extern "C" int dinox_surface_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values,
                                   int64_t* bad, void* ws, int64_t B, int H, int W, int C, int T, int q_num, int q_den, void* stream) {
  DX_REQUIRE(pred && gt && spacing && tol && counts && values && bad && ws, DINOX_EINVAL, "surface_stats: null pointer");
  DX_REQUIRE(H >= 1 && H <= dinox::SURF_MAX_SIDE && W >= 1 && W <= dinox::SURF_MAX_SIDE, DINOX_EINVAL, "surface_stats: H=%d W=%d (1 <= H, W <= %d)", H, W,
             dinox::SURF_MAX_SIDE);
  DX_REQUIRE(C >= 2 && C <= dinox::SEG_MAX_CLASSES, DINOX_EINVAL, "surface_stats: C=%d (2 <= C <= %d)", C, dinox::SEG_MAX_CLASSES);
  DX_REQUIRE(surface_sizes_ok(B, H, W, C), DINOX_EINVAL, "surface_stats: B=%lld (B >= 1 and B C 2 H <= 2^30; evaluate a longer batch in pieces)",
             (long long)B);
  DX_REQUIRE(T >= 1 && T <= dinox::SURF_MAX_TOL, DINOX_EINVAL, "surface_stats: T=%d tolerances (1 <= T <= %d)", T, dinox::SURF_MAX_TOL);
  for (int t = 0; t < T; ++t) DX_REQUIRE(tol[t] >= 0.f && tol[t] <= 3.0e38f, DINOX_EINVAL, "surface_stats: tolerance %d is %g (finite and >= 0)", t, (double)tol[t]);
  DX_REQUIRE(q_num > 0 && q_num <= q_den, DINOX_EINVAL, "surface_stats: quantile %d/%d (0 < q_num <= q_den)", q_num, q_den);
  return dinox::launch_surface_stats(pred, gt, spacing, tol, counts, values, bad, ws, B, H, W, C, T, q_num, q_den, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- connected components of a label map (kernels: cclabel.hip)
// B H W < 2^31: every pixel index of an image fits int32 (and 20 bits: H, W <= 1024), every batch offset int64.
static bool cc_sizes_ok(int64_t B, int H, int W, int C) {
  return B >= 1 && B < ((int64_t)1 << 31) && H >= 1 && H <= dinox::CC_MAX_SIDE && W >= 1 && W <= dinox::CC_MAX_SIDE && C >= 2 &&
         C <= dinox::SEG_MAX_CLASSES && B * H * W < ((int64_t)1 << 31);
}

#define DX_CC_SIZES(what)                                                                                                                        \
  do {                                                                                                                                           \
    DX_REQUIRE(H >= 1 && H <= dinox::CC_MAX_SIDE && W >= 1 && W <= dinox::CC_MAX_SIDE, DINOX_EINVAL, what ": H=%d W=%d (1 <= H, W <= %d)", H, W, \
               dinox::CC_MAX_SIDE);                                                                                                              \
    DX_REQUIRE(C >= 2 && C <= dinox::SEG_MAX_CLASSES, DINOX_EINVAL, what ": C=%d (2 <= C <= %d)", C, dinox::SEG_MAX_CLASSES);                     \
    DX_REQUIRE(cc_sizes_ok(B, H, W, C), DINOX_EINVAL, what ": B=%lld (B >= 1 and B H W < 2^31; cut a longer batch in pieces)", (long long)B);     \
  } while (0)

extern "C" int64_t dinox_cc_ws_bytes(int64_t B, int H, int W, int C) { return cc_sizes_ok(B, H, W, C) ? dinox::cc_ws_bytes(B, H, W, C) : 0; }

extern "C" int dinox_cc_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t B,
                              int H, int W, int C, int connectivity, void* stream) {
  DX_REQUIRE(labels && comp && area && ncomp && bad && ws, DINOX_EINVAL, "cc_label: null pointer");
  DX_CC_SIZES("cc_label");
  DX_REQUIRE(connectivity == 4 || connectivity == 8, DINOX_EINVAL, "cc_label: connectivity=%d (4 or 8)", connectivity);
  return dinox::launch_cc_label(labels, mask, comp, area, ncomp, bad, ws, B, H, W, C, connectivity, dinox::as_stream(stream));
}

extern "C" int dinox_cc_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, const uint8_t* y, uint8_t* out,
                               int64_t* counts, void* ws, int64_t B, int H, int W, int C, int c0, int keep_largest, void* stream) {
  DX_REQUIRE(labels && comp && area && out && ws, DINOX_EINVAL, "cc_filter: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "cc_filter: y and counts go together (both or neither)");
  DX_CC_SIZES("cc_filter");
  DX_REQUIRE(c0 >= 0 && c0 <= C, DINOX_EINVAL, "cc_filter: c0=%d (0 <= c0 <= C = %d)", c0, C);
  return dinox::launch_cc_filter(labels, comp, area, min_px, y, out, counts, ws, B, H, W, C, c0, keep_largest ? 1 : 0, dinox::as_stream(stream));
}

extern "C" int dinox_cc_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                              const int32_t* gt_area, const int32_t* min_px, int64_t* counts, void* ws, int64_t B, int H, int W, int C, int t_num,
                              int t_den, void* stream) {
  DX_REQUIRE(pred && pred_comp && pred_area && gt && gt_comp && gt_area && counts && ws, DINOX_EINVAL, "cc_match: null pointer");
  DX_CC_SIZES("cc_match");
  DX_REQUIRE(t_den > 0 && t_den < (1 << 20) && t_num >= 0 && t_num <= t_den, DINOX_EINVAL,
             "cc_match: overlap %d/%d (0 <= t_num <= t_den, 0 < t_den < 2^20)", t_num, t_den);
  return dinox::launch_cc_match(pred, pred_comp, pred_area, gt, gt_comp, gt_area, min_px, counts, ws, B, H, W, C, t_num, t_den, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- connected components of one label volume (kernels: cclabel3d.hip)
// Z H W <= 2^30: every voxel index and every area fits int32.
static bool cc3d_sizes_ok(int64_t Z, int H, int W, int C) {
  return Z >= 1 && Z <= dinox::CC3D_MAX_VOXELS && H >= 1 && H <= dinox::CC_MAX_SIDE && W >= 1 && W <= dinox::CC_MAX_SIDE && C >= 2 &&
         C <= dinox::SEG_MAX_CLASSES && Z * H * W <= dinox::CC3D_MAX_VOXELS;
}

#define DX_CC3D_SIZES(what)                                                                                                                      \
  do {                                                                                                                                           \
    DX_REQUIRE(H >= 1 && H <= dinox::CC_MAX_SIDE && W >= 1 && W <= dinox::CC_MAX_SIDE, DINOX_EINVAL, what ": H=%d W=%d (1 <= H, W <= %d)", H, W, \
               dinox::CC_MAX_SIDE);                                                                                                              \
    DX_REQUIRE(C >= 2 && C <= dinox::SEG_MAX_CLASSES, DINOX_EINVAL, what ": C=%d (2 <= C <= %d)", C, dinox::SEG_MAX_CLASSES);                     \
    DX_REQUIRE(cc3d_sizes_ok(Z, H, W, C), DINOX_EINVAL, what ": Z=%lld (Z >= 1 and Z H W <= 2^30; label a longer series in pieces)", (long long)Z); \
  } while (0)

extern "C" int64_t dinox_cc3d_ws_bytes(int64_t Z, int H, int W, int C) { return cc3d_sizes_ok(Z, H, W, C) ? dinox::cc3d_ws_bytes(Z, H, W, C) : 0; }

extern "C" int dinox_cc3d_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t Z,
                                int H, int W, int C, int connectivity, void* stream) {
  DX_REQUIRE(labels && comp && area && ncomp && bad && ws, DINOX_EINVAL, "cc3d_label: null pointer");
  DX_CC3D_SIZES("cc3d_label");
  DX_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, DINOX_EINVAL, "cc3d_label: connectivity=%d (6, 18 or 26)", connectivity);
  return dinox::launch_cc3d_label(labels, mask, comp, area, ncomp, bad, ws, Z, H, W, C, connectivity, dinox::as_stream(stream));
}

extern "C" int dinox_cc3d_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, int min_vox, const uint8_t* y, uint8_t* out,
                                 int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int c0, int keep_largest, void* stream) {
  DX_REQUIRE(labels && comp && area && out && ws, DINOX_EINVAL, "cc3d_filter: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "cc3d_filter: y and counts go together (both or neither)");
  DX_CC3D_SIZES("cc3d_filter");
  DX_REQUIRE(min_vox >= 0, DINOX_EINVAL, "cc3d_filter: min_vox=%d (>= 0)", min_vox);
  DX_REQUIRE(c0 >= 0 && c0 <= C, DINOX_EINVAL, "cc3d_filter: c0=%d (0 <= c0 <= C = %d)", c0, C);
  return dinox::launch_cc3d_filter(labels, comp, area, min_vox, y, out, counts, ws, Z, H, W, C, c0, keep_largest ? 1 : 0, dinox::as_stream(stream));
}

extern "C" int dinox_cc3d_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                                const int32_t* gt_area, int min_vox, int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int t_num, int t_den,
                                void* stream) {
  DX_REQUIRE(pred && pred_comp && pred_area && gt && gt_comp && gt_area && counts && ws, DINOX_EINVAL, "cc3d_match: null pointer");
  DX_CC3D_SIZES("cc3d_match");
  DX_REQUIRE(min_vox >= 0, DINOX_EINVAL, "cc3d_match: min_vox=%d (>= 0)", min_vox);
  DX_REQUIRE(t_den > 0 && t_den < (1 << 20) && t_num >= 0 && t_num <= t_den, DINOX_EINVAL,
             "cc3d_match: overlap %d/%d (0 <= t_num <= t_den, 0 < t_den < 2^20)", t_num, t_den);
  return dinox::launch_cc3d_match(pred, pred_comp, pred_area, gt, gt_comp, gt_area, min_vox, counts, ws, Z, H, W, C, t_num, t_den, dinox::as_stream(stream));
}

// ---------------------------------------------------------------- LoRA low-rank products (kernels: lora.hip)
static bool lora_rank_ok(int r) { return r >= 1 && r <= dinox::LORA_MAX_RANK; }
static bool lora_dim_ok(int d) { return d >= 1 && d <= (1 << 20); }
static bool lora_rows_ok(int64_t M) { return M >= 1 && M <= 0x7fffffff; }

extern "C" int dinox_lora_down(const void* x, const float* small, float* u, int64_t M, int K, int r, int small_layout, int dtype, void* stream) {
  DX_REQUIRE(x && small && u, DINOX_EINVAL, "lora_down: null pointer");
  DX_REQUIRE(mae_dtype_ok(dtype) && (small_layout == 0 || small_layout == 1), DINOX_EINVAL, "lora_down: dtype %d, small_layout %d", dtype,
             small_layout);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_down: r=%d (1 <= r <= %d)", r, dinox::LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(K), DINOX_EINVAL, "lora_down: M=%lld K=%d (1 <= M <= 2^31 - 1; 1 <= K <= 2^20)", (long long)M, K);
  return dinox::launch_lora_down(x, small, u, M, K, r, small_layout, dtype, dinox::as_stream(stream));
}

extern "C" int dinox_lora_up(const float* u, const float* small, const float* res, float* t, float s, int64_t M, int N, int r, int small_layout,
                             void* stream) {
  DX_REQUIRE(u && small && t, DINOX_EINVAL, "lora_up: null pointer");
  DX_REQUIRE(small_layout == 0 || small_layout == 1, DINOX_EINVAL, "lora_up: small_layout %d", small_layout);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_up: r=%d (1 <= r <= %d)", r, dinox::LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(N) && dinox::lora_up_grid_ok(M, N), DINOX_EINVAL,
             "lora_up: M=%lld N=%d (1 <= M <= 2^31 - 1; 1 <= N <= 2^20; M N / 4 <= 2^39)", (long long)M, N);
  return dinox::launch_lora_up(u, small, res, t, s, M, N, r, small_layout, dinox::as_stream(stream));
}

extern "C" int64_t dinox_lora_grad_ws_bytes(int64_t M, int K, int N, int r) {
  if (!(lora_rows_ok(M) && lora_dim_ok(K) && lora_dim_ok(N) && lora_rank_ok(r))) return 0;
  return dinox::lora_grad_chunks(M) * ((int64_t)r * K + (int64_t)N * r) * (int64_t)sizeof(float);
}

extern "C" int dinox_lora_grad(const void* xl, const void* dy, const float* A, const float* B, float s, float* dA, float* dB, float* ws, int64_t M,
                               int K, int N, int r, int dtype, void* stream) {
  DX_REQUIRE(xl && dy && A && B && dA && dB && ws, DINOX_EINVAL, "lora_grad: null pointer");
  DX_REQUIRE(mae_dtype_ok(dtype), DINOX_EINVAL, "lora_grad: dtype %d", dtype);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_grad: r=%d (1 <= r <= %d)", r, dinox::LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(K) && lora_dim_ok(N), DINOX_EINVAL, "lora_grad: M=%lld K=%d N=%d (1 <= M <= 2^31 - 1; 1 <= K, N <= 2^20)",
             (long long)M, K, N);
  return dinox::launch_lora_grad(xl, dy, A, B, s, dA, dB, ws, M, K, N, r, dtype, dinox::as_stream(stream));
}

extern "C" int dinox_lora_dropout(const void* in, void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  DX_REQUIRE(in && out, DINOX_EINVAL, "lora_dropout: null pointer");
  DX_REQUIRE(mae_dtype_ok(dtype), DINOX_EINVAL, "lora_dropout: dtype %d", dtype);
  DX_REQUIRE(p >= 0.f && p < 1.f, DINOX_EINVAL, "lora_dropout: p=%g outside [0, 1)", (double)p);
  DX_REQUIRE(n >= 1 && n <= ((int64_t)1 << 40), DINOX_EINVAL, "lora_dropout: n=%lld (1 <= n <= 2^40)", (long long)n);
  return dinox::launch_lora_dropout(in, out, n, p, seed, offset, dtype, dinox::as_stream(stream));
}

extern "C" int dinox_lora_merge(const float* w, const float* A, const float* B, float* w_out, float s, int sign, int N, int K, int r, void* stream) {
  DX_REQUIRE(w && A && B && w_out, DINOX_EINVAL, "lora_merge: null pointer");
  DX_REQUIRE(sign == 1 || sign == -1, DINOX_EINVAL, "lora_merge: sign %d (+1 merges, -1 unmerges)", sign);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_merge: r=%d (1 <= r <= %d)", r, dinox::LORA_MAX_RANK);
  DX_REQUIRE(lora_dim_ok(N) && lora_dim_ok(K) && dinox::lora_up_grid_ok(N, K), DINOX_EINVAL, "lora_merge: N=%d K=%d (1 <= N, K <= 2^20)", N, K);
  // w_out[n][k] = w[n][k] + (sign s) sum_j B[n][j] A[j][k]: the up product with B as its rows and A stored [r][K]
  return dinox::launch_lora_up(B, A, w, w_out, (float)sign * s, N, K, r, 1, dinox::as_stream(stream));
}
