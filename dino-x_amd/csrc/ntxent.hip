// ntxent.hip -- NT-Xent (SimCLR) loss head on the student head output.
// Replaces SimCLRLoss.forward of the reference (scripts/phase5_big_run.py:776-813, used at :1728-1737) and its autograd backward:
//     z^ = F.normalize(z) over the M = 2B rows [z1; z2];  s = z^ z^T / tau with the diagonal excluded;
//     loss = mean_i ( logsumexp_{j != i} s_ij - s_{i p(i)} ),   p(i) = (i + B) mod 2B.
// The two M x M x D products (S = Z^ Z^T and dZ^ = W Z^) go through dinox_gemm (exact-fp32 MFMA) and the row normalisation through
// dinox_koleo_normalize (same formula, eps is an argument); here: the row pass over S, the coefficient matrix W of the backward and
// the backward of the normalisation.  Under data parallelism the rows are this rank's and the columns every rank's: the
// rectangular forms below (ntxent_rows_rect / ntxent_coeff_rect), [Ml, Mg] instead of [M, M].
//
// Documented deviation: everything is fp32 in BOTH compute modes (as KoLeo).  Under --amp the reference's autocast runs the
// similarity matmul in bf16; this engine stays at fp32 there, i.e. closer to the reference's own fp32 step.
// No float atomics: every sum has a fixed order, so a step is bit-reproducible.
#include "small_common.h"

namespace dinox {

constexpr int NX_THREADS = 256;
constexpr int NX_TILE = 32;

// One workgroup per row i of S: lse[i] = logsumexp_{j != i} S[i][j] * inv_tau, row_loss[i] = lse[i] - S[i][p(i)] * inv_tau.
// Skipping the diagonal equals the reference's -9e15 fill: exp(-9e15 - max) is 0 in fp32.
__global__ __launch_bounds__(NX_THREADS) void ntxent_rows_kernel(const float* __restrict__ S, int64_t lds, int M, float inv_tau,
                                                                 float* __restrict__ lse, float* __restrict__ row_loss) {
  __shared__ float red[16];
  const int i = blockIdx.x;
  const float* row = S + (int64_t)i * lds;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < M; j += NX_THREADS)
    if (j != i) mx = fmaxf(mx, row[j] * inv_tau);
  mx = block_max(mx, red);
  float a = 0.f;
  for (int j = threadIdx.x; j < M; j += NX_THREADS)
    if (j != i) a += expf(row[j] * inv_tau - mx);
  a = block_sum(a, red);
  if (threadIdx.x == 0) {
    const int p = i + (M >> 1) < M ? i + (M >> 1) : i - (M >> 1);
    const float l = mx + logf(a);
    lse[i] = l;
    row_loss[i] = l - row[p] * inv_tau;
  }
}

// out[0] = (sum_i row_loss[i]) / divisor, added in index order by one thread; the rows pass through LDS in chunks so that the loads are
// one coalesced sweep and the serial chain is M dependent adds on LDS reads (M = 512: ~2 us).  divisor = M gives the loss; the
// rectangular form passes 1 (an exact division) for the plain sum: the ranks' sums meet on the host side of the all-gather, which
// divides by Mg once.
__global__ __launch_bounds__(NX_THREADS) void ntxent_sum_kernel(const float* __restrict__ row_loss, int M, float divisor, float* __restrict__ out) {
  __shared__ float buf[1024];
  float a = 0.f;
  for (int base = 0; base < M; base += 1024) {
    const int n = M - base < 1024 ? M - base : 1024;
    for (int t = threadIdx.x; t < n; t += NX_THREADS) buf[t] = row_loss[base + t];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int t = 0; t < n; ++t) a += buf[t];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = a / divisor;
}

// W[i][j] = scale * (exp(S_ij/tau - lse_i) + exp(S_ji/tau - lse_j) - [j = p(i)] - [i = p(j)]),  W[i][i] = 0,  scale = g / (M tau).
// One workgroup per 32 x 32 tile: it reads the tile and its mirror image (S_ji through LDS, so both reads are coalesced); the GEMM
// output is not assumed to be bit-symmetric.  W is a separate buffer: the workgroup of the mirror tile reads what this one would
// overwrite.
__global__ __launch_bounds__(NX_THREADS) void ntxent_coeff_kernel(const float* __restrict__ S, int64_t lds, const float* __restrict__ lse,
                                                                  int M, float inv_tau, float scale, float* __restrict__ W, int64_t ldw) {
  __shared__ float mir[NX_TILE][NX_TILE + 1];
  const int tx = threadIdx.x & (NX_TILE - 1), ty = threadIdx.x >> 5;  // 32 x 8
  const int i0 = blockIdx.y * NX_TILE, j0 = blockIdx.x * NX_TILE, half = M >> 1;
  for (int r = ty; r < NX_TILE; r += NX_THREADS / NX_TILE) {           // mir[r][c] = S[j0 + r][i0 + c]
    const int jj = j0 + r, ii = i0 + tx;
    mir[r][tx] = (jj < M && ii < M) ? S[(int64_t)jj * lds + ii] : 0.f;
  }
  __syncthreads();
  const int j = j0 + tx;
  if (j >= M) return;
  const float lj = lse[j];
  for (int r = ty; r < NX_TILE; r += NX_THREADS / NX_TILE) {
    const int i = i0 + r;
    if (i >= M) break;
    float w = 0.f;
    if (i != j) {
      const int pi = i + half < M ? i + half : i - half, pj = j + half < M ? j + half : j - half;
      w = expf(S[(int64_t)i * lds + j] * inv_tau - lse[i]) + expf(mir[tx][r] * inv_tau - lj);
      w -= (j == pi ? 1.f : 0.f) + (i == pj ? 1.f : 0.f);
      w *= scale;
    }
    W[(int64_t)i * ldw + j] = w;
  }
}

// ---------------------------------------------------------------- rectangular forms: local rows x global columns (data parallel)
// A rank holds Ml = 2 Bl rows [z1_local; z2_local]; S [Ml, Mg] is their product with the Mg = world * Ml gathered rows, rank r's
// block starting at column row0 = r * Ml.  For local row i the excluded column is its own global index dg(i) = row0 + i and its
// positive is p(i) = row0 + (i + Bl) mod Ml.  The square kernels above stay as they are (same device code, same bits); with
// Mg = Ml and row0 = 0 these compute the same lse from the same S.
__device__ __forceinline__ int ntxent_rect_pos(int i, int row0, int Bl) { return row0 + (i + Bl < 2 * Bl ? i + Bl : i - Bl); }

__global__ __launch_bounds__(NX_THREADS) void ntxent_rows_rect_kernel(const float* __restrict__ S, int64_t lds, int Mg, int row0, int Bl,
                                                                      float inv_tau, float* __restrict__ lse, float* __restrict__ row_loss) {
  __shared__ float red[16];
  const int i = blockIdx.x, dg = row0 + i;
  const float* row = S + (int64_t)i * lds;
  float mx = -INFINITY;
  for (int j = threadIdx.x; j < Mg; j += NX_THREADS)
    if (j != dg) mx = fmaxf(mx, row[j] * inv_tau);
  mx = block_max(mx, red);
  float a = 0.f;
  for (int j = threadIdx.x; j < Mg; j += NX_THREADS)
    if (j != dg) a += expf(row[j] * inv_tau - mx);
  a = block_sum(a, red);
  if (threadIdx.x == 0) {
    const float l = mx + logf(a);
    lse[i] = l;
    row_loss[i] = l - row[ntxent_rect_pos(i, row0, Bl)] * inv_tau;
  }
}

// W[i][j] = scale * (exp(S_ij/tau - lse_local[i]) + exp(S_ij/tau - lse_all[j]) - 2 [j = p(i)]),  W[i][dg(i)] = 0,  scale = g / (Ml tau).
// The second term is P_ji: S_ji lives on the rank that owns row j, so S_ij stands in for it (the product is symmetric up to rounding)
// with the gathered lse of row j; [i = p(j)] = [j = p(i)] for this pairing.  One workgroup per 32 x 32 tile, every element read and
// written by one thread: no mirror tile, no LDS.
__global__ __launch_bounds__(NX_THREADS) void ntxent_coeff_rect_kernel(const float* __restrict__ S, int64_t lds,
                                                                       const float* __restrict__ lse_local, const float* __restrict__ lse_all,
                                                                       int Ml, int Mg, int row0, int Bl, float inv_tau, float scale,
                                                                       float* __restrict__ W, int64_t ldw) {
  const int tx = threadIdx.x & (NX_TILE - 1), ty = threadIdx.x >> 5;  // 32 x 8
  const int i0 = blockIdx.y * NX_TILE, j = blockIdx.x * NX_TILE + tx;
  if (j >= Mg) return;
  const float lj = lse_all[j];
  for (int r = ty; r < NX_TILE; r += NX_THREADS / NX_TILE) {
    const int i = i0 + r;
    if (i >= Ml) break;
    float w = 0.f;
    if (j != row0 + i) {
      const float s = S[(int64_t)i * lds + j] * inv_tau;
      w = expf(s - lse_local[i]) + expf(s - lj);
      w -= j == ntxent_rect_pos(i, row0, Bl) ? 2.f : 0.f;
      w *= scale;
    }
    W[(int64_t)i * ldw + j] = w;
  }
}

// Backward of xh = x / max(||x||, eps), one workgroup per row:  dx = (dxh - xh (xh . dxh)) / ||x||  where ||x|| >= eps, and
// dx = dxh / eps where the clamp acted (what torch's clamp_min + norm backward give: no gradient reaches the norm there).
template <bool VEC>
__global__ __launch_bounds__(NX_THREADS) void normalize_bwd_kernel(const float* __restrict__ dxh, const float* __restrict__ xh,
                                                                   const float* __restrict__ norm, float* __restrict__ dx, int D, float eps) {
  __shared__ float red[16];
  const int64_t r = blockIdx.x;
  const float* g = dxh + r * D;
  const float* u = xh + r * D;
  float* o = dx + r * D;
  const int D4 = VEC ? D >> 2 : 0;
  float dot = 0.f;
  for (int q = threadIdx.x; q < D4; q += NX_THREADS) {
    const float4 gv = reinterpret_cast<const float4*>(g)[q], uv = reinterpret_cast<const float4*>(u)[q];
    dot += gv.x * uv.x + gv.y * uv.y + gv.z * uv.z + gv.w * uv.w;
  }
  for (int d = 4 * D4 + threadIdx.x; d < D; d += NX_THREADS) dot += g[d] * u[d];
  dot = block_sum(dot, red);
  const float n = norm[r];
  const bool clamped = n < eps;
  const float inv = 1.0f / (clamped ? eps : n), c = clamped ? 0.f : dot;
  for (int q = threadIdx.x; q < D4; q += NX_THREADS) {
    const float4 gv = reinterpret_cast<const float4*>(g)[q], uv = reinterpret_cast<const float4*>(u)[q];
    reinterpret_cast<float4*>(o)[q] = make_float4((gv.x - uv.x * c) * inv, (gv.y - uv.y * c) * inv, (gv.z - uv.z * c) * inv, (gv.w - uv.w * c) * inv);
  }
  for (int d = 4 * D4 + threadIdx.x; d < D; d += NX_THREADS) o[d] = (g[d] - u[d] * c) * inv;
}

}  // namespace dinox

using namespace dinox;

static bool ntxent_rows_ok(int M) { return M >= 2 && M % 2 == 0 && M <= 65535 * 32; }

extern "C" int dinox_ntxent_rows(const float* S, int64_t lds, int M, float inv_tau, float* lse, float* row_loss, float* loss, void* stream) {
  DX_REQUIRE(S && lse && row_loss && loss, DINOX_EINVAL, "ntxent_rows: null pointer");
  DX_REQUIRE(ntxent_rows_ok(M), DINOX_EINVAL, "ntxent_rows: M=%d (the rows are [z1; z2]: an even count of at least 2)", M);
  DX_REQUIRE(lds >= M && inv_tau > 0.f, DINOX_EINVAL, "ntxent_rows: lds=%lld M=%d inv_tau=%g", (long long)lds, M, (double)inv_tau);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ntxent_rows_kernel, dim3((unsigned)M), dim3(NX_THREADS), 0, st, S, lds, M, inv_tau, lse, row_loss);
  const int rc = check_launch("ntxent_rows");
  if (rc) return rc;
  hipLaunchKernelGGL(ntxent_sum_kernel, dim3(1), dim3(NX_THREADS), 0, st, row_loss, M, (float)M, loss);
  return check_launch("ntxent_rows_mean");
}

extern "C" int dinox_ntxent_coeff(const float* S, int64_t lds, const float* lse, int M, float inv_tau, float gscale, float* W, int64_t ldw,
                                  void* stream) {
  DX_REQUIRE(S && lse && W, DINOX_EINVAL, "ntxent_coeff: null pointer");
  DX_REQUIRE(ntxent_rows_ok(M), DINOX_EINVAL, "ntxent_coeff: M=%d (the rows are [z1; z2]: an even count of at least 2)", M);
  DX_REQUIRE(lds >= M && ldw >= M && inv_tau > 0.f, DINOX_EINVAL, "ntxent_coeff: lds=%lld ldw=%lld M=%d inv_tau=%g", (long long)lds,
             (long long)ldw, M, (double)inv_tau);
  DX_REQUIRE(W != S, DINOX_EINVAL, "ntxent_coeff: W must not alias S (a tile reads its mirror image, which another workgroup writes)");
  const unsigned tiles = (unsigned)ceil_div(M, NX_TILE);
  const float scale = gscale * inv_tau / (float)M;
  hipLaunchKernelGGL(ntxent_coeff_kernel, dim3(tiles, tiles), dim3(NX_THREADS), 0, as_stream(stream), S, lds, lse, M, inv_tau, scale, W, ldw);
  return check_launch("ntxent_coeff");
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
  int rc = ntxent_rect_ok("ntxent_rows_rect", lds, Ml, Mg, row0, Bl, inv_tau);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ntxent_rows_rect_kernel, dim3((unsigned)Ml), dim3(NX_THREADS), 0, st, S, lds, Mg, row0, Bl, inv_tau, lse, row_loss);
  rc = check_launch("ntxent_rows_rect");
  if (rc) return rc;
  hipLaunchKernelGGL(ntxent_sum_kernel, dim3(1), dim3(NX_THREADS), 0, st, row_loss, Ml, 1.0f, loss_sum);
  return check_launch("ntxent_rows_rect_sum");
}

extern "C" int dinox_ntxent_coeff_rect(const float* S, int64_t lds, const float* lse_local, const float* lse_all, int Ml, int Mg, int row0,
                                       int Bl, float inv_tau, float gscale, float* W, int64_t ldw, void* stream) {
  DX_REQUIRE(S && lse_local && lse_all && W, DINOX_EINVAL, "ntxent_coeff_rect: null pointer");
  const int rc = ntxent_rect_ok("ntxent_coeff_rect", lds, Ml, Mg, row0, Bl, inv_tau);
  if (rc) return rc;
  DX_REQUIRE(ldw >= Mg, DINOX_EINVAL, "ntxent_coeff_rect: ldw=%lld Mg=%d", (long long)ldw, Mg);
  const float scale = gscale * inv_tau / (float)Ml;
  hipLaunchKernelGGL(ntxent_coeff_rect_kernel, dim3((unsigned)ceil_div(Mg, NX_TILE), (unsigned)ceil_div(Ml, NX_TILE)), dim3(NX_THREADS), 0,
                     as_stream(stream), S, lds, lse_local, lse_all, Ml, Mg, row0, Bl, inv_tau, scale, W, ldw);
  return check_launch("ntxent_coeff_rect");
}

extern "C" int dinox_normalize_bwd(const float* dxh, const float* xh, const float* norm, float* dx, int64_t V, int D, float eps, void* stream) {
  DX_REQUIRE(dxh && xh && norm && dx, DINOX_EINVAL, "normalize_bwd: null pointer");
  DX_REQUIRE(V > 0 && V <= 0x7fffffff && D > 0 && eps > 0.f, DINOX_EINVAL, "normalize_bwd: V=%lld D=%d eps=%g", (long long)V, D, (double)eps);
  hipStream_t st = as_stream(stream);
  const bool vec = D % 4 == 0 && aligned16(dxh, xh, dx);
  if (vec) hipLaunchKernelGGL(normalize_bwd_kernel<true>, dim3((unsigned)V), dim3(NX_THREADS), 0, st, dxh, xh, norm, dx, D, eps);
  else hipLaunchKernelGGL(normalize_bwd_kernel<false>, dim3((unsigned)V), dim3(NX_THREADS), 0, st, dxh, xh, norm, dx, D, eps);
  return check_launch("normalize_bwd");
}
