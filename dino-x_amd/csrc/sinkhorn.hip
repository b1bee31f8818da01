// sinkhorn.hip -- Sinkhorn-Knopp teacher centring (DINOv2/v3) as a centre vector for the DINO cross-entropy kernels of loss.hip.
// An extension: the reference trains with the EMA centre only (DINOLoss.update_center, scripts/phase5_big_run.py:686-720).
//
// With z[i][k] = t[i][k] / tau the published loop (normalise exp(z)^T by its sum, then n times: over prototypes, over samples) ends on
// Q[i][:] = softmax_k(z[i][k] + b_n[k]), where, in the log domain,
//     a_0 = 0,   b_n[k] = -log sum_i exp(z[i][k] + a_{n-1}[i]),   a_n[i] = -log sum_k exp(z[i][k] + b_n[k]),
// i.e. the targets dino_ce_kernel already forms from the centre c = -tau b_n.  Everything here is fp32 and max-shifted: no exp of an
// unshifted logit (at tau = 0.04 exp(z) leaves fp32 at a logit of 3.6).  Every result is a pure function of the inputs: fixed
// reduction trees, partials met in index order, no atomics.
#include "small_common.h"

namespace dinox {

constexpr int SK_THREADS = 256;
constexpr int SK_CHUNK = 32;   // rows of one column-pass workgroup: 512 rows x 8192 columns = 16 x 32 workgroups (colmean_kernel's layout: 32)

// ---------------------------------------------------------------- column pass, stage 1: (max, sum exp) of a chunk of rows
// A workgroup owns 64 float4 column groups and SK_CHUNK rows; its four 64-thread slices take interleaved rows (8 each, loaded once and
// held in registers for both the max and the sum) and meet in LDS in slice order.  A row past the end enters as -inf: exp gives an exact 0.
template <bool HAS_A>
__global__ __launch_bounds__(SK_THREADS) void sk_col_partial_kernel(const float* __restrict__ t, const float* __restrict__ a, float inv,
                                                                    float* __restrict__ pm, float* __restrict__ ps, int R, int K) {
  __shared__ float4 part[4][64];
  constexpr int PER = SK_CHUNK / 4;
  const int K4 = K / 4, lane = threadIdx.x & 63, c4 = blockIdx.x * 64 + lane, slice = threadIdx.x >> 6;
  const int r0 = blockIdx.y * SK_CHUNK + slice;
  const bool live = c4 < K4;
  float4 x[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int r = r0 + 4 * j;
    if (live && r < R) {
      const float4 v = *reinterpret_cast<const float4*>(t + (int64_t)r * K + (int64_t)c4 * 4);
      const float ar = HAS_A ? a[r] : 0.f;
      x[j] = make_float4(fmaf(v.x, inv, ar), fmaf(v.y, inv, ar), fmaf(v.z, inv, ar), fmaf(v.w, inv, ar));
    } else {
      x[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
  }
  float4 m = x[0];
#pragma unroll
  for (int j = 1; j < PER; ++j) m = make_float4(fmaxf(m.x, x[j].x), fmaxf(m.y, x[j].y), fmaxf(m.z, x[j].z), fmaxf(m.w, x[j].w));
  part[slice][lane] = m;
  __syncthreads();
  const float4 m0 = part[0][lane], m1 = part[1][lane], m2 = part[2][lane], m3 = part[3][lane];
  m = make_float4(fmaxf(fmaxf(m0.x, m1.x), fmaxf(m2.x, m3.x)), fmaxf(fmaxf(m0.y, m1.y), fmaxf(m2.y, m3.y)),
                  fmaxf(fmaxf(m0.z, m1.z), fmaxf(m2.z, m3.z)), fmaxf(fmaxf(m0.w, m1.w), fmaxf(m2.w, m3.w)));
  __syncthreads();
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {      // (the chunk's first row exists, so m is finite here)
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      s.x += expf(x[j].x - m.x); s.y += expf(x[j].y - m.y); s.z += expf(x[j].z - m.z); s.w += expf(x[j].w - m.w);
    }
  }
  part[slice][lane] = s;
  __syncthreads();
  if (slice == 0 && live) {
    const float4 p0 = part[0][lane], p1 = part[1][lane], p2 = part[2][lane], p3 = part[3][lane];
    const int64_t o = (int64_t)blockIdx.y * K + (int64_t)c4 * 4;
    *reinterpret_cast<float4*>(pm + o) = m;
    *reinterpret_cast<float4*>(ps + o) = make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y),
                                                     (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
  }
}

// any K / alignment: one thread per column, the chunk's rows in order
template <bool HAS_A>
__global__ __launch_bounds__(SK_THREADS) void sk_col_partial_scalar_kernel(const float* __restrict__ t, const float* __restrict__ a, float inv,
                                                                           float* __restrict__ pm, float* __restrict__ ps, int R, int K) {
  const int k = blockIdx.x * SK_THREADS + threadIdx.x;
  if (k >= K) return;
  const int r0 = blockIdx.y * SK_CHUNK, r1 = min(R, r0 + SK_CHUNK);
  float m = -INFINITY;
  for (int r = r0; r < r1; ++r) m = fmaxf(m, fmaf(t[(int64_t)r * K + k], inv, HAS_A ? a[r] : 0.f));
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += expf(fmaf(t[(int64_t)r * K + k], inv, HAS_A ? a[r] : 0.f) - m);
  pm[(int64_t)blockIdx.y * K + k] = m;
  ps[(int64_t)blockIdx.y * K + k] = s;
}

// ---------------------------------------------------------------- column pass, stage 2: the chunks of a column, in chunk order
// out[k] = oscale * (M + log sum_c ps[c][k] exp(pm[c][k] - M)),  M = max_c pm[c][k]
__global__ __launch_bounds__(SK_THREADS) void sk_col_combine_kernel(const float* __restrict__ pm, const float* __restrict__ ps, float oscale,
                                                                    float* __restrict__ out, int chunks, int K) {
  const int k = blockIdx.x * SK_THREADS + threadIdx.x;
  if (k >= K) return;
  float m = pm[k];
  for (int c = 1; c < chunks; ++c) m = fmaxf(m, pm[(int64_t)c * K + k]);
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += ps[(int64_t)c * K + k] * expf(pm[(int64_t)c * K + k] - m);
  out[k] = oscale * (m + logf(s));
}

// ---------------------------------------------------------------- row pass: one workgroup per row, as the cross-entropy kernels
// out[i] = oscale * log sum_k exp(t[i][k] inv + b[k]).  VEC: K % 4 == 0 and 16-byte aligned t and b.
template <bool VEC, bool HAS_B>
__global__ __launch_bounds__(SK_THREADS) void sk_row_lse_kernel(const float* __restrict__ t, const float* __restrict__ b, float inv, float oscale,
                                                                float* __restrict__ out, int K) {
  __shared__ float red[16];
  const float* tr = t + (int64_t)blockIdx.x * K;
  float m = -INFINITY, s = 0.f;
  if (VEC) {
    const int K4 = K / 4;
    for (int k = threadIdx.x; k < K4; k += SK_THREADS) {
      const float4 v = reinterpret_cast<const float4*>(tr)[k];
      const float4 bb = HAS_B ? reinterpret_cast<const float4*>(b)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
      m = fmaxf(fmaxf(m, fmaxf(fmaf(v.x, inv, bb.x), fmaf(v.y, inv, bb.y))), fmaxf(fmaf(v.z, inv, bb.z), fmaf(v.w, inv, bb.w)));
    }
    m = block_max(m, red);
    for (int k = threadIdx.x; k < K4; k += SK_THREADS) {
      const float4 v = reinterpret_cast<const float4*>(tr)[k];
      const float4 bb = HAS_B ? reinterpret_cast<const float4*>(b)[k] : make_float4(0.f, 0.f, 0.f, 0.f);
      s += expf(fmaf(v.x, inv, bb.x) - m);
      s += expf(fmaf(v.y, inv, bb.y) - m);
      s += expf(fmaf(v.z, inv, bb.z) - m);
      s += expf(fmaf(v.w, inv, bb.w) - m);
    }
  } else {
    for (int k = threadIdx.x; k < K; k += SK_THREADS) m = fmaxf(m, fmaf(tr[k], inv, HAS_B ? b[k] : 0.f));
    m = block_max(m, red);
    for (int k = threadIdx.x; k < K; k += SK_THREADS) s += expf(fmaf(tr[k], inv, HAS_B ? b[k] : 0.f) - m);
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = oscale * (m + logf(s));
}

static inline int sk_chunks(int R) { return (int)ceil_div(R, SK_CHUNK); }

static int sk_check(const char* what, const void* t, const void* out, int R, int K) {
  DX_REQUIRE(t && out, DINOX_EINVAL, "%s: null pointer", what);
  DX_REQUIRE(R >= 1 && K >= 1, DINOX_EINVAL, "%s: R=%d K=%d (both must be >= 1)", what, R, K);
  return 0;
}

// the column pass puts its chunks on grid.y
static int sk_col_check(const char* what, const void* ws, int R) {
  DX_REQUIRE(ws, DINOX_EINVAL, "%s: null workspace", what);
  DX_REQUIRE(sk_chunks(R) <= 65535, DINOX_EINVAL, "%s: R=%d is more than %d rows", what, R, 65535 * SK_CHUNK);
  return 0;
}

static int sk_col_launch(const float* t, const float* a, float inv, float oscale, float* out, float* ws, int R, int K, hipStream_t st) {
  const int chunks = sk_chunks(R);
  float* pm = ws;                              // [chunks][K]
  float* ps = ws + (int64_t)chunks * K;        // [chunks][K]
  if (K % 4 == 0 && aligned16(t, ws)) {
    const dim3 grid((unsigned)ceil_div(K / 4, 64), (unsigned)chunks);
    if (a) hipLaunchKernelGGL((sk_col_partial_kernel<true>), grid, dim3(SK_THREADS), 0, st, t, a, inv, pm, ps, R, K);
    else hipLaunchKernelGGL((sk_col_partial_kernel<false>), grid, dim3(SK_THREADS), 0, st, t, a, inv, pm, ps, R, K);
  } else {
    const dim3 grid((unsigned)ceil_div(K, SK_THREADS), (unsigned)chunks);
    if (a) hipLaunchKernelGGL((sk_col_partial_scalar_kernel<true>), grid, dim3(SK_THREADS), 0, st, t, a, inv, pm, ps, R, K);
    else hipLaunchKernelGGL((sk_col_partial_scalar_kernel<false>), grid, dim3(SK_THREADS), 0, st, t, a, inv, pm, ps, R, K);
  }
  int rc = check_launch("sk_col_partial");
  if (rc) return rc;
  hipLaunchKernelGGL(sk_col_combine_kernel, dim3((unsigned)ceil_div(K, SK_THREADS)), dim3(SK_THREADS), 0, st, pm, ps, oscale, out, chunks, K);
  return check_launch("sk_col_combine");
}

static int sk_row_launch(const float* t, const float* b, float inv, float oscale, float* out, int R, int K, hipStream_t st) {
  const bool vec = K % 4 == 0 && aligned16(t, b);
  const dim3 grid((unsigned)R), block(SK_THREADS);
  if (vec && b) hipLaunchKernelGGL((sk_row_lse_kernel<true, true>), grid, block, 0, st, t, b, inv, oscale, out, K);
  else if (vec) hipLaunchKernelGGL((sk_row_lse_kernel<true, false>), grid, block, 0, st, t, b, inv, oscale, out, K);
  else if (b) hipLaunchKernelGGL((sk_row_lse_kernel<false, true>), grid, block, 0, st, t, b, inv, oscale, out, K);
  else hipLaunchKernelGGL((sk_row_lse_kernel<false, false>), grid, block, 0, st, t, b, inv, oscale, out, K);
  return check_launch("sk_row_lse");
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_sk_ws_floats(int R, int K) {
  if (R < 1 || K < 1) return 0;
  return 2 * (int64_t)sk_chunks(R) * K + K + R;
}

extern "C" int dinox_sk_col_lse(const float* t, const float* a, float inv_temp, float out_scale, float* out, float* ws, int R, int K,
                                void* stream) {
  int rc = sk_check("sk_col_lse", t, out, R, K);
  if (!rc) rc = sk_col_check("sk_col_lse", ws, R);
  if (rc) return rc;
  return sk_col_launch(t, a, inv_temp, out_scale, out, ws, R, K, as_stream(stream));
}

extern "C" int dinox_sk_row_lse(const float* t, const float* b, float inv_temp, float out_scale, float* out, int R, int K, void* stream) {
  int rc = sk_check("sk_row_lse", t, out, R, K);
  if (rc) return rc;
  return sk_row_launch(t, b, inv_temp, out_scale, out, R, K, as_stream(stream));
}

extern "C" int dinox_sk_center(const float* t, float teacher_temp, int n_iters, float* center_out, float* ws, int R, int K, void* stream) {
  int rc = sk_check("sk_center", t, center_out, R, K);
  if (!rc) rc = sk_col_check("sk_center", ws, R);
  if (rc) return rc;
  DX_REQUIRE(n_iters >= 1, DINOX_EINVAL, "sk_center: n_iters=%d (must be >= 1)", n_iters);
  DX_REQUIRE(teacher_temp > 0.f, DINOX_EINVAL, "sk_center: teacher_temp must be > 0");
  hipStream_t st = as_stream(stream);
  const float inv = 1.0f / teacher_temp;
  float* b = ws + 2 * (int64_t)sk_chunks(R) * K;     // [K]  (16-byte aligned with ws when K % 4 == 0: the row pass keeps its float4 path)
  float* a = b + K;                                  // [R]
  for (int n = 1; n <= n_iters; ++n) {
    const bool last = n == n_iters;                  // centre = -tau b = tau lse
    rc = sk_col_launch(t, n == 1 ? nullptr : a, inv, last ? teacher_temp : -1.0f, last ? center_out : b, ws, R, K, st);
    if (rc || last) return rc;
    rc = sk_row_launch(t, b, inv, -1.0f, a, R, K, st);
    if (rc) return rc;
  }
  return 0;
}
