// ibot.hip -- the masked-patch (iBOT / DINOv2) objective's kernels.  An extension: the reference trains with the image-level DINO term only.
//     put_mask          patches[idx[m]][:] = mask_token, in place on the patch product's output (the student sees a learned token there)
//     put_mask_bwd      dmask_token = sum_m dpatches[idx[m]][:], then those rows of dpatches = 0 (no gradient into the patch product)
//     gather_rows       dst[dst_row0 + m] = src[row[m]]: the masked patch tokens of the final features, appended to the head's CLS operand
//     scatter_add_rows  dst[row[m]] += src[src_row0 + m]: the head's input gradient back into the feature gradient (rows distinct)
//     ibot_center_ema   the patch centre's EMA from (column sums, row count) -- what the ranks add up under data parallelism
//     ibot_ce           centring / sharpening cross-entropy of M unpaired rows with per-row weights, loss and d loss / d logits
// fp32 math.  No float atomics: every sum has a fixed order (stated at each kernel), so a step is bit-reproducible.  Every index read from
// device memory is range-checked before it becomes an address; an entry outside is skipped.
#include "small_common.h"

namespace dinox {

constexpr int IB_THREADS = 256;
constexpr int IBOT_MASK_CHUNK = 64;        // masked rows per partial sum of put_mask_bwd: ws holds ceil(M / 64) x D floats
constexpr int IBOT_CE_REG_MAX_K = 8192;    // widest row the register-resident cross-entropy holds: 8 float4 per thread and matrix

// ---------------------------------------------------------------- mask token in / out of the patch rows
template <int DT>
__global__ __launch_bounds__(IB_THREADS) void ibot_put_mask_kernel(void* __restrict__ patches, const float* __restrict__ mask_token,
                                                                   const int* __restrict__ idx, int M, int64_t rows, int D) {
  const int64_t total = (int64_t)M * D;
  for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * IB_THREADS) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    const int64_t r = idx[m];
    if (r < 0 || r >= rows) continue;
    elem<DT>::st(patches, r * D + d, mask_token[d]);
  }
}

// ws[c][d] = sum of dpatches[idx[m]][d] over the m of chunk c = [c CH, min(M, (c + 1) CH)), ascending m: one thread per (chunk, feature).
template <int DT>
__global__ __launch_bounds__(IB_THREADS) void ibot_mask_partial_kernel(const void* __restrict__ dpatches, const int* __restrict__ idx,
                                                                       float* __restrict__ ws, int M, int64_t rows, int D) {
  const int d = blockIdx.x * IB_THREADS + threadIdx.x, c = blockIdx.y;
  if (d >= D) return;
  const int m0 = c * IBOT_MASK_CHUNK, m1 = min(M, m0 + IBOT_MASK_CHUNK);
  float acc = 0.f;
  for (int m = m0; m < m1; ++m) {
    const int64_t r = idx[m];
    if (r < 0 || r >= rows) continue;
    acc += elem<DT>::ld(dpatches, r * D + d);
  }
  ws[(int64_t)c * D + d] = acc;
}

// One launch, two roles, both after every partial was read.  The first `sum_blocks` workgroups: dmask[d] = sum_c ws[c][d], ascending c
// (a chain of ceil(M / CH) fp32 adds on top of the chunk's CH).  The remaining workgroups set the masked rows of dpatches to 0.
template <int DT>
__global__ __launch_bounds__(IB_THREADS) void ibot_mask_combine_kernel(void* __restrict__ dpatches, const int* __restrict__ idx,
                                                                       const float* __restrict__ ws, float* __restrict__ dmask, int M,
                                                                       int64_t rows, int D, int chunks, int sum_blocks) {
  if ((int)blockIdx.x < sum_blocks) {
    const int d = blockIdx.x * IB_THREADS + threadIdx.x;
    if (d >= D) return;
    float acc = 0.f;
    for (int c = 0; c < chunks; ++c) acc += ws[(int64_t)c * D + d];
    dmask[d] = acc;
    return;
  }
  const int64_t total = (int64_t)M * D, nb = gridDim.x - sum_blocks;
  for (int64_t i = (int64_t)(blockIdx.x - sum_blocks) * IB_THREADS + threadIdx.x; i < total; i += nb * IB_THREADS) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    const int64_t r = idx[m];
    if (r < 0 || r >= rows) continue;
    elem<DT>::st(dpatches, r * D + d, 0.f);
  }
}

// ---------------------------------------------------------------- indexed row gather / scatter-add
template <int DT>
__global__ __launch_bounds__(IB_THREADS) void gather_rows_kernel(const float* __restrict__ src, const int* __restrict__ row, void* __restrict__ dst,
                                                                 int64_t M, int64_t src_rows, int D, int64_t dst_row0) {
  const int64_t total = M * D;
  for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * IB_THREADS) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    const int64_t r = row[m];
    if (r < 0 || r >= src_rows) continue;
    elem<DT>::st(dst, (dst_row0 + m) * D + d, src[r * D + d]);
  }
}

// dst[row[m]][d] += src[src_row0 + m][d]: one fp32 add per element; the rows are distinct by contract, so no two threads meet.
template <int DT>
__global__ __launch_bounds__(IB_THREADS) void scatter_add_rows_kernel(const void* __restrict__ src, const int* __restrict__ row,
                                                                      float* __restrict__ dst, int64_t M, int64_t dst_rows, int D,
                                                                      int64_t src_row0) {
  const int64_t total = M * D;
  for (int64_t i = (int64_t)blockIdx.x * IB_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * IB_THREADS) {
    const int64_t m = i / D;
    const int d = (int)(i - m * D);
    const int64_t r = row[m];
    if (r < 0 || r >= dst_rows) continue;
    dst[r * D + d] += elem<DT>::ld(src, (src_row0 + m) * D + d);
  }
}

// ---------------------------------------------------------------- cross-entropy of M unpaired rows
// One workgroup per row m, log-sum-exp form throughout as dino_ce_kernel (loss.hip), with the same operations per element:
//     zs = s / ts - max,   p_t = exp((t - c) / tt - max) / sum,   row_loss = -sum_k p_t (zs - log sum exp zs),
//     ds = g_m (exp(zs) / sum - p_t) / ts,   g_m = gscale * w[m]  (one rounded multiply).
// Register-resident form: thread i holds float4 groups i, i + 256, ... of the row (NV of them per matrix: K <= 1024 NV), each loaded ONCE
// and already scaled; the max, the sum and the output pass read registers, so s, t and ds cross the memory bus once each.  At K = 8192
// that is 64 VGPRs of row data per lane (128 allocated, no scratch: 4 waves per SIMD, i.e. 4 rows in flight per CU; 256 threads keep the
// block reductions at four waves).  A group past the row's end holds -inf and is left out of the output pass.
template <int NV>
__global__ __launch_bounds__(IB_THREADS) void ibot_ce_reg_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                                 const float* __restrict__ center, const float* __restrict__ w, float inv_ts,
                                                                 float inv_tt, float gscale, float* __restrict__ ds,
                                                                 float* __restrict__ row_loss, int K4) {
  __shared__ float red[16];
  const int64_t base = (int64_t)blockIdx.x * K4;
  const float4* sr = reinterpret_cast<const float4*>(s) + base;
  const float4* tr = reinterpret_cast<const float4*>(t) + base;
  const float4* cr = reinterpret_cast<const float4*>(center);
  float4 zs[NV], zt[NV];
  float ms = -INFINITY, mt = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int k = threadIdx.x + j * IB_THREADS;
    if (k < K4) {
      const float4 a = sr[k], b = tr[k], c = cr[k];
      zs[j] = make_float4(a.x * inv_ts, a.y * inv_ts, a.z * inv_ts, a.w * inv_ts);
      zt[j] = make_float4((b.x - c.x) * inv_tt, (b.y - c.y) * inv_tt, (b.z - c.z) * inv_tt, (b.w - c.w) * inv_tt);
    } else {
      zs[j] = zt[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    }
    ms = fmaxf(fmaxf(ms, fmaxf(zs[j].x, zs[j].y)), fmaxf(zs[j].z, zs[j].w));
    mt = fmaxf(fmaxf(mt, fmaxf(zt[j].x, zt[j].y)), fmaxf(zt[j].z, zt[j].w));
  }
  ms = block_max(ms, red);
  mt = block_max(mt, red);
  float ss = 0.f, st = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {      // (zs becomes the shifted logit, zt the unnormalised target: exp(-inf) is an exact 0)
    zs[j] = make_float4(zs[j].x - ms, zs[j].y - ms, zs[j].z - ms, zs[j].w - ms);
    zt[j] = make_float4(expf(zt[j].x - mt), expf(zt[j].y - mt), expf(zt[j].z - mt), expf(zt[j].w - mt));
    ss += expf(zs[j].x); ss += expf(zs[j].y); ss += expf(zs[j].z); ss += expf(zs[j].w);
    st += zt[j].x; st += zt[j].y; st += zt[j].z; st += zt[j].w;
  }
  ss = block_sum(ss, red);
  st = block_sum(st, red);
  const float log_ss = logf(ss), inv_ss = 1.0f / ss, inv_st = 1.0f / st;
  const float g = gscale * w[blockIdx.x];
  float4* dr = ds ? reinterpret_cast<float4*>(ds) + base : nullptr;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int k = threadIdx.x + j * IB_THREADS;
    if (k >= K4) continue;
    const float4 tp = make_float4(zt[j].x * inv_st, zt[j].y * inv_st, zt[j].z * inv_st, zt[j].w * inv_st);
    acc -= tp.x * (zs[j].x - log_ss); acc -= tp.y * (zs[j].y - log_ss); acc -= tp.z * (zs[j].z - log_ss); acc -= tp.w * (zs[j].w - log_ss);
    if (dr)
      store_stream(dr + k, make_float4(g * (expf(zs[j].x) * inv_ss - tp.x) * inv_ts, g * (expf(zs[j].y) * inv_ss - tp.y) * inv_ts,
                                       g * (expf(zs[j].z) * inv_ss - tp.z) * inv_ts, g * (expf(zs[j].w) * inv_ss - tp.w) * inv_ts));
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) row_loss[blockIdx.x] = acc;
}

// Any K and alignment: three passes over the row (the re-reads come from L2).
__global__ __launch_bounds__(IB_THREADS) void ibot_ce_scalar_kernel(const float* __restrict__ s, const float* __restrict__ t,
                                                                    const float* __restrict__ center, const float* __restrict__ w, float inv_ts,
                                                                    float inv_tt, float gscale, float* __restrict__ ds,
                                                                    float* __restrict__ row_loss, int K) {
  __shared__ float red[16];
  const int64_t base = (int64_t)blockIdx.x * K;
  const float* sr = s + base;
  const float* tr = t + base;
  float ms = -INFINITY, mt = -INFINITY;
  for (int k = threadIdx.x; k < K; k += IB_THREADS) {
    ms = fmaxf(ms, sr[k] * inv_ts);
    mt = fmaxf(mt, (tr[k] - center[k]) * inv_tt);
  }
  ms = block_max(ms, red);
  mt = block_max(mt, red);
  float ss = 0.f, st = 0.f;
  for (int k = threadIdx.x; k < K; k += IB_THREADS) {
    ss += expf(sr[k] * inv_ts - ms);
    st += expf((tr[k] - center[k]) * inv_tt - mt);
  }
  ss = block_sum(ss, red);
  st = block_sum(st, red);
  const float log_ss = logf(ss), inv_ss = 1.0f / ss, inv_st = 1.0f / st;
  const float g = gscale * w[blockIdx.x];
  float acc = 0.f;
  for (int k = threadIdx.x; k < K; k += IB_THREADS) {
    const float zs = sr[k] * inv_ts - ms;
    const float tp = expf((tr[k] - center[k]) * inv_tt - mt) * inv_st;
    acc -= tp * (zs - log_ss);
    if (ds) ds[base + k] = g * (expf(zs) * inv_ss - tp) * inv_ts;
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) row_loss[blockIdx.x] = acc;
}

// loss[0] = scale * sum_m w[m] row_loss[m]: thread i adds rows i, i + 256, ... in ascending order, then block_sum (a fixed order).
__global__ __launch_bounds__(IB_THREADS) void ibot_weighted_sum_kernel(const float* __restrict__ row_loss, const float* __restrict__ w, int M,
                                                                       float scale, float* __restrict__ loss) {
  __shared__ float red[16];
  const float a = block_strided_sum(row_loss, w, M, red);
  if (threadIdx.x == 0) loss[0] = a * scale;
}

// center[k] = center[k] mom + (sum_count[k] / sum_count[K]) (1 - mom): the mean of the masked teacher rows from their column sums and
// their number (element K, a whole number held in fp32), both possibly summed over ranks.  A count below 1 leaves the centre untouched.
__global__ __launch_bounds__(IB_THREADS) void ibot_center_ema_kernel(float* __restrict__ c, const float* __restrict__ sum_count, float mom, int K) {
  const int k = blockIdx.x * IB_THREADS + threadIdx.x;
  const float n = sum_count[K];
  if (k < K && n >= 1.0f) c[k] = c[k] * mom + (sum_count[k] / n) * (1.0f - mom);
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// M masked rows out of `rows` (flat int32 positions), D features.
static bool ibot_rows_ok(int64_t M, int64_t rows, int D) {
  return M >= 1 && M <= 0x7fffffff && rows >= 1 && rows <= 0x7fffffff && D >= 1 && D <= (1 << 16);
}

extern "C" int dinox_ibot_put_mask(void* patches, const float* mask_token, const int* idx, int M, int64_t rows, int D, int dtype, void* stream) {
  DX_REQUIRE(patches && mask_token && idx, DINOX_EINVAL, "ibot_put_mask: null pointer");
  DX_REQUIRE(dtype_ok(dtype), DINOX_EINVAL, "ibot_put_mask: dtype %d", dtype);
  DX_REQUIRE(ibot_rows_ok(M, rows, D), DINOX_EINVAL, "ibot_put_mask: M=%d rows=%lld D=%d (M, rows >= 1; 1 <= D <= 65536)", M, (long long)rows, D);
  DX_LAUNCH_DT(ibot_put_mask_kernel, dtype, dim3(grid_1d((int64_t)M * D, IB_THREADS, 4096)), dim3(IB_THREADS), as_stream(stream), patches, mask_token, idx,
               M, rows, D);
  return check_launch("ibot_put_mask");
}

extern "C" int dinox_ibot_put_mask_bwd(void* dpatches, const int* idx, float* dmask_token, float* ws, int M, int64_t rows, int D, int dtype,
                                       void* stream) {
  DX_REQUIRE(dpatches && idx && dmask_token && ws, DINOX_EINVAL, "ibot_put_mask_bwd: null pointer");
  DX_REQUIRE(dtype_ok(dtype), DINOX_EINVAL, "ibot_put_mask_bwd: dtype %d", dtype);
  DX_REQUIRE(ibot_rows_ok(M, rows, D) && M <= 65535 * IBOT_MASK_CHUNK, DINOX_EINVAL,
             "ibot_put_mask_bwd: M=%d rows=%lld D=%d (1 <= M <= %d; rows >= 1; 1 <= D <= 65536)", M, (long long)rows, D, 65535 * IBOT_MASK_CHUNK);
  hipStream_t st = as_stream(stream);
  const int chunks = (int)ceil_div(M, IBOT_MASK_CHUNK), col_blocks = (int)ceil_div(D, IB_THREADS);
  DX_LAUNCH_DT(ibot_mask_partial_kernel, dtype, dim3((unsigned)col_blocks, (unsigned)chunks), dim3(IB_THREADS), st, dpatches, idx, ws, M, rows, D);
  int rc = check_launch("ibot_put_mask_bwd");
  if (rc) return rc;
  const dim3 grid((unsigned)col_blocks + grid_1d((int64_t)M * D, IB_THREADS, 4096));
  DX_LAUNCH_DT(ibot_mask_combine_kernel, dtype, grid, dim3(IB_THREADS), st, dpatches, idx, ws, dmask_token, M, rows, D, chunks, col_blocks);
  return check_launch("ibot_put_mask_bwd_combine");
}

extern "C" int dinox_gather_rows(const float* src, const int* row, void* dst, int64_t M, int64_t src_rows, int D, int64_t dst_row0, int dst_dtype,
                                 void* stream) {
  DX_REQUIRE(src && row && dst, DINOX_EINVAL, "gather_rows: null pointer");
  DX_REQUIRE(dtype_ok(dst_dtype), DINOX_EINVAL, "gather_rows: dtype %d", dst_dtype);
  DX_REQUIRE(ibot_rows_ok(M, src_rows, D) && dst_row0 >= 0, DINOX_EINVAL, "gather_rows: M=%lld src_rows=%lld D=%d dst_row0=%lld", (long long)M,
             (long long)src_rows, D, (long long)dst_row0);
  DX_LAUNCH_DT(gather_rows_kernel, dst_dtype, dim3(grid_1d(M * D, IB_THREADS, 4096)), dim3(IB_THREADS), as_stream(stream), src, row, dst, M, src_rows, D,
               dst_row0);
  return check_launch("gather_rows");
}

extern "C" int dinox_scatter_add_rows(const void* src, const int* row, float* dst, int64_t M, int64_t dst_rows, int D, int64_t src_row0,
                                      int src_dtype, void* stream) {
  DX_REQUIRE(src && row && dst, DINOX_EINVAL, "scatter_add_rows: null pointer");
  DX_REQUIRE(dtype_ok(src_dtype), DINOX_EINVAL, "scatter_add_rows: dtype %d", src_dtype);
  DX_REQUIRE(ibot_rows_ok(M, dst_rows, D) && src_row0 >= 0, DINOX_EINVAL, "scatter_add_rows: M=%lld dst_rows=%lld D=%d src_row0=%lld", (long long)M,
             (long long)dst_rows, D, (long long)src_row0);
  DX_LAUNCH_DT(scatter_add_rows_kernel, src_dtype, dim3(grid_1d(M * D, IB_THREADS, 4096)), dim3(IB_THREADS), as_stream(stream), src, row, dst, M, dst_rows,
               D, src_row0);
  return check_launch("scatter_add_rows");
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
  hipStream_t st = as_stream(stream);
  const float inv_ts = 1.0f / student_temp, inv_tt = 1.0f / teacher_temp, gscale = grad_scale * scale;
  const bool reg = K % 4 == 0 && K <= IBOT_CE_REG_MAX_K && aligned16(s, t, center, ds);
  const dim3 grid((unsigned)M), block(IB_THREADS);
  if (reg) {
    const int K4 = K / 4, nv = (int)ceil_div(K4, IB_THREADS);
#define IB_CE(NV) hipLaunchKernelGGL((ibot_ce_reg_kernel<NV>), grid, block, 0, st, s, t, center, w, inv_ts, inv_tt, gscale, ds, row_loss, K4)
    if (nv <= 1) IB_CE(1);
    else if (nv <= 2) IB_CE(2);
    else if (nv <= 4) IB_CE(4);
    else IB_CE(8);
#undef IB_CE
  } else {
    hipLaunchKernelGGL(ibot_ce_scalar_kernel, grid, block, 0, st, s, t, center, w, inv_ts, inv_tt, gscale, ds, row_loss, K);
  }
  int rc = check_launch("ibot_ce");
  if (rc) return rc;
  hipLaunchKernelGGL(ibot_weighted_sum_kernel, dim3(1), block, 0, st, row_loss, w, M, scale, loss);
  return check_launch("ibot_ce_sum");
}

extern "C" int dinox_ibot_center_ema(float* center, const float* sum_count, float momentum, int K, void* stream) {
  DX_REQUIRE(center && sum_count && K >= 1, DINOX_EINVAL, "ibot_center_ema: bad arguments");
  hipLaunchKernelGGL(ibot_center_ema_kernel, dim3((unsigned)ceil_div(K, IB_THREADS)), dim3(IB_THREADS), 0, as_stream(stream), center, sum_count, momentum, K);
  return check_launch("ibot_center_ema");
}
