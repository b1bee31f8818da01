// mae.hip -- the masked-token glue of the MAE objective (reference scripts/phase5_big_run.py: MaeModel.random_masking / forward /
// patchify / forward_loss and MaeDecoder.forward's un-shuffle), one pass each instead of argsort x 2, gather x 3, repeat, cat x 2, an
// einsum-patchified copy of the batch and a [V, L, 3 p^2] squared-error tensor:
//     mask_ids        noise [V, L] -> ids_restore (stable rank of every patch), ids_keep (the Lk patches of lowest noise, in rank order)
//     gather_unfold   the patch-embed operand of the KEPT patches only ([V Lk, cols]; rows v L + ids_keep of dinox_patch_unfold(_ld))
//     tokens          [cls + pos[0] | patches[r] + pos[1 + ids_keep[r]]]  and its backward (dpos is a gather over ids_restore)
//     unshuffle       decoder input: kept rows back in place, mask_token elsewhere, + the fixed sin-cos table; and its backward
//     loss            mean over removed patches of the mean squared error against pixels read straight from the image
// All memory-bound.  No float atomics: every sum has a fixed order (the chains are stated at each kernel), so a step is bit-reproducible.
// Every index read from device memory (ids_keep, ids_restore) is range-checked before it becomes an address.
#include "small_common.h"

namespace dinox {

constexpr int MAE_THREADS = 256;
constexpr int MAE_MAX_L = 4096;      // patches per sample: the sort keys of one sample sit in LDS
constexpr int MAE_MAX_PATCH = 32;    // patch edge of the loss kernels: one target patch (3 p^2 floats) sits in LDS

__device__ __forceinline__ int clamp_idx(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// ---------------------------------------------------------------- mask ids
// A key whose unsigned order is the order torch.argsort uses: -0 == +0, every NaN equal and above +inf.  With ties broken by index the
// ranks are a permutation of 0 .. L-1 for ANY input, so ids_keep is always written completely and holds valid patch numbers.
__device__ __forceinline__ uint32_t order_key(float f) {
  if (f != f) return 0xffffffffu;
  const uint32_t u = __float_as_uint(f + 0.0f);        // (-0) + (+0) = +0; every other value unchanged
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// One workgroup per sample: the L keys sit in LDS, thread p counts the keys below its own (every lane reads the same LDS word: a broadcast).
__global__ __launch_bounds__(MAE_THREADS) void mae_mask_ids_kernel(const float* __restrict__ noise, int* __restrict__ ids_restore,
                                                                   int* __restrict__ ids_keep, int L, int Lk) {
  __shared__ uint32_t key[MAE_MAX_L];
  const int64_t v = blockIdx.x;
  for (int p = threadIdx.x; p < L; p += MAE_THREADS) key[p] = order_key(noise[v * L + p]);
  __syncthreads();
  for (int p = threadIdx.x; p < L; p += MAE_THREADS) {
    const uint32_t k = key[p];
    int r = 0;
    for (int q = 0; q < L; ++q) {
      const uint32_t kq = key[q];
      r += (kq < k || (kq == k && q < p)) ? 1 : 0;
    }
    ids_restore[v * L + p] = r;
    if (r < Lk) ids_keep[v * Lk + r] = p;
  }
}

// ---------------------------------------------------------------- gather + unfold
// u[(v Lk + r)][c p p + py p + px] = x[v][c][gy p + py][gx p + px] for patch l = ids_keep[v][r] = gy g + gx; columns 3 p^2 .. ld-1 are 0.
// VW = 4 (p % 4 == 0): one thread moves 4 consecutive px.
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_gather_unfold_kernel(const float* __restrict__ x, const int* __restrict__ ids_keep,
                                                                        void* __restrict__ u, int V, int H, int W, int p, int Lk, int ld) {
  const int g = W / p, L = g * (H / p), Kd = 3 * p * p, ldv = ld / VW;
  const int64_t total = (int64_t)V * Lk * ldv;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(idx % ldv) * VW;
    const int64_t row = idx / ldv;
    fvec<VW> val = vzero<VW>();
    if (k < Kd) {
      const int64_t v = row / Lk;
      const int l = clamp_idx(ids_keep[row], L);
      const int gx = l % g, gy = l / g;
      const int px = k % p, py = (k / p) % p, c = k / (p * p);
      val = ld_f32<VW>(x + ((v * 3 + c) * H + (gy * p + py)) * (int64_t)W + gx * p + px);
    }
    st_dt<DT, VW>(u, row * ld + k, val);
  }
}

// ---------------------------------------------------------------- encoder tokens
// tok[v][0] = cls + pos[0];  tok[v][1 + r] = patches[v][r] + pos[1 + ids_keep[v][r]]   (one fp32 add per element)
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_tokens_fwd_kernel(const void* __restrict__ patches, const float* __restrict__ cls,
                                                                     const float* __restrict__ pos, const int* __restrict__ ids_keep,
                                                                     float* __restrict__ tok, int V, int L, int Lk, int D) {
  const int N = 1 + Lk, DV = D / VW;
  const int64_t total = (int64_t)V * N * DV;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int dd = (int)(idx % DV) * VW;
    const int64_t t2 = idx / DV;
    const int n = (int)(t2 % N);
    const int64_t v = t2 / N;
    fvec<VW> val;
    if (n == 0) {
      val = vadd<VW>(ld_f32<VW>(cls + dd), ld_f32<VW>(pos + dd));
    } else {
      const int64_t row = v * Lk + (n - 1);
      const int l = clamp_idx(ids_keep[row], L);
      val = vadd<VW>(ld_dt<DT, VW>(patches, row * D + dd), ld_f32<VW>(pos + (int64_t)(1 + l) * D + dd));
    }
    st_f32<VW>(tok + (v * N + n) * D + dd, val);
  }
}

// One launch, two roles.  The first (1 + L) * chunks workgroups own one position n and 256 feature groups each:
//     dpos[0] = dcls = sum_v dtok[v][0];   dpos[1 + p] = sum over the v with r = ids_restore[v][p] < Lk of dtok[v][1 + r]
// added in ascending v by one thread (a chain of at most V fp32 adds; about V (Lk / L) of them for a patch position) -- a gather
// driven by ids_restore, no scatter-add.  The remaining workgroups copy dpatches[v][r] = dtok[v][1 + r] in the operand dtype.
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_tokens_bwd_kernel(const float* __restrict__ dtok, const int* __restrict__ ids_restore,
                                                                     void* __restrict__ dpatches, float* __restrict__ dcls,
                                                                     float* __restrict__ dpos, int V, int L, int Lk, int D, int chunks,
                                                                     int param_blocks) {
  const int N = 1 + Lk, DV = D / VW;
  if ((int)blockIdx.x < param_blocks) {
    const int n = blockIdx.x / chunks, c = (blockIdx.x % chunks) * MAE_THREADS + threadIdx.x;
    if (c >= DV) return;
    const int dd = c * VW;
    fvec<VW> acc = vzero<VW>();
    for (int v = 0; v < V; ++v) {
      int row = 0;
      if (n > 0) {
        const int r = ids_restore[(int64_t)v * L + (n - 1)];
        if (r < 0 || r >= Lk) continue;
        row = 1 + r;
      }
      acc = vadd<VW>(acc, ld_f32<VW>(dtok + ((int64_t)v * N + row) * D + dd));
    }
    st_f32<VW>(dpos + (int64_t)n * D + dd, acc);
    if (n == 0) st_f32<VW>(dcls + dd, acc);
    return;
  }
  const int64_t total = (int64_t)V * Lk * DV, nb = gridDim.x - param_blocks;
  for (int64_t idx = (int64_t)(blockIdx.x - param_blocks) * blockDim.x + threadIdx.x; idx < total; idx += nb * blockDim.x) {
    const int dd = (int)(idx % DV) * VW;
    const int64_t t2 = idx / DV;
    const int r = (int)(t2 % Lk);
    const int64_t v = t2 / Lk;
    st_dt<DT, VW>(dpatches, (v * Lk + r) * D + dd, ld_f32<VW>(dtok + (v * N + 1 + r) * D + dd));
  }
}

// ---------------------------------------------------------------- decoder un-shuffle
// xd[v][0] = e[v][0] + dpe[0];  xd[v][1 + p] = (r = ids_restore[v][p]) < Lk ? e[v][1 + r] : mask_token, + dpe[1 + p]   (one fp32 add)
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_unshuffle_fwd_kernel(const void* __restrict__ e, const float* __restrict__ mask_token,
                                                                        const float* __restrict__ dpe, const int* __restrict__ ids_restore,
                                                                        float* __restrict__ xd, int V, int L, int Lk, int D) {
  const int N = 1 + L, Ne = 1 + Lk, DV = D / VW;
  const int64_t total = (int64_t)V * N * DV;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int dd = (int)(idx % DV) * VW;
    const int64_t t2 = idx / DV;
    const int n = (int)(t2 % N);
    const int64_t v = t2 / N;
    fvec<VW> val;
    if (n == 0) {
      val = ld_dt<DT, VW>(e, v * Ne * D + dd);
    } else {
      const int r = ids_restore[v * L + (n - 1)];
      val = (r >= 0 && r < Lk) ? ld_dt<DT, VW>(e, (v * Ne + 1 + r) * D + dd) : ld_f32<VW>(mask_token + dd);
    }
    st_f32<VW>(xd + (v * N + n) * D + dd, vadd<VW>(val, ld_f32<VW>(dpe + (int64_t)n * D + dd)));
  }
}

// One launch, two roles.  The first V * chunks workgroups own one sample and 256 feature groups each:
//     part[v] = sum over the removed patches p of sample v (ids_restore[v][p] outside [0, Lk)) of g[v][1 + p],  ascending p
// (a chain of L - Lk fp32 adds).  The remaining workgroups gather de[v][0] = g[v][0], de[v][1 + r] = g[v][1 + ids_keep[v][r]].
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_unshuffle_bwd_kernel(const float* __restrict__ g, const int* __restrict__ ids_keep,
                                                                        const int* __restrict__ ids_restore, void* __restrict__ de,
                                                                        float* __restrict__ part, int V, int L, int Lk, int D, int chunks,
                                                                        int part_blocks) {
  const int N = 1 + L, Ne = 1 + Lk, DV = D / VW;
  if ((int)blockIdx.x < part_blocks) {
    const int v = blockIdx.x / chunks, c = (blockIdx.x % chunks) * MAE_THREADS + threadIdx.x;
    if (c >= DV) return;
    const int dd = c * VW;
    fvec<VW> acc = vzero<VW>();
    for (int p = 0; p < L; ++p) {
      const int r = ids_restore[(int64_t)v * L + p];
      if (r >= 0 && r < Lk) continue;
      acc = vadd<VW>(acc, ld_f32<VW>(g + ((int64_t)v * N + 1 + p) * D + dd));
    }
    st_f32<VW>(part + (int64_t)v * D + dd, acc);
    return;
  }
  const int64_t total = (int64_t)V * Ne * DV, nb = gridDim.x - part_blocks;
  for (int64_t idx = (int64_t)(blockIdx.x - part_blocks) * blockDim.x + threadIdx.x; idx < total; idx += nb * blockDim.x) {
    const int dd = (int)(idx % DV) * VW;
    const int64_t t2 = idx / DV;
    const int n = (int)(t2 % Ne);
    const int64_t v = t2 / Ne;
    const int src = n == 0 ? 0 : 1 + clamp_idx(ids_keep[v * Lk + (n - 1)], L);
    st_dt<DT, VW>(de, (v * Ne + n) * D + dd, ld_f32<VW>(g + (v * N + src) * D + dd));
  }
}

// dmask[d] = sum_v part[v][d], ascending v (a chain of V fp32 adds), one thread per feature group.
template <int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_colsum_rows_kernel(const float* __restrict__ part, float* __restrict__ out, int V, int D) {
  const int c = blockIdx.x * MAE_THREADS + threadIdx.x;
  if (c >= D / VW) return;
  const int dd = c * VW;
  fvec<VW> acc = vzero<VW>();
  for (int v = 0; v < V; ++v) acc = vadd<VW>(acc, ld_f32<VW>(part + (int64_t)v * D + dd));
  st_f32<VW>(out + dd, acc);
}

// ---------------------------------------------------------------- reconstruction loss
// The target patch of (v, l), in patchify order j = (py p + px) 3 + c, staged in LDS: the image is read along px (contiguous), the LDS
// writes have stride 3 words (no bank conflict), and pred is then read along j.
__device__ __forceinline__ void mae_stage_target(const float* __restrict__ x, float* tgt, int64_t v, int l, int H, int W, int p) {
  const int g = W / p, gx = l % g, gy = l / g, K = 3 * p * p;
  for (int t = threadIdx.x; t < K; t += MAE_THREADS) {
    const int px = t % p, py = (t / p) % p, c = t / (p * p);
    tgt[(py * p + px) * 3 + c] = x[((v * 3 + c) * H + (gy * p + py)) * (int64_t)W + gx * p + px];
  }
  __syncthreads();
}

// One workgroup per (v, l).  pred is [V][lead + L][3 p^2] (lead = 1: the CLS row of the decoder output is still in front).
// row_loss[v L + l] = mean_j (pred - target)^2 on a removed patch, exactly 0 on a kept one.  Each thread adds its j, j + 256 VW, ... in
// ascending order, then the wave / workgroup tree of block_sum: a fixed order.
template <int DT, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_rows_kernel(const void* __restrict__ pred, const float* __restrict__ x,
                                                                    const int* __restrict__ ids_restore, float* __restrict__ row_loss,
                                                                    int H, int W, int p, int Lk, int lead) {
  __shared__ float tgt[3 * MAE_MAX_PATCH * MAE_MAX_PATCH];
  __shared__ float red[16];
  const int L = (W / p) * (H / p), K = 3 * p * p;
  const int64_t v = blockIdx.x / L;
  const int l = blockIdx.x % L;
  const int r = ids_restore[v * L + l];
  if (r >= 0 && r < Lk) {                                 // (uniform over the workgroup)
    if (threadIdx.x == 0) row_loss[blockIdx.x] = 0.f;
    return;
  }
  mae_stage_target(x, tgt, v, l, H, W, p);
  const int64_t base = (v * (lead + L) + lead + l) * K;
  float acc = 0.f;
  for (int j = threadIdx.x * VW; j < K; j += MAE_THREADS * VW) {
    const fvec<VW> q = ld_dt<DT, VW>(pred, base + j);
#pragma unroll
    for (int i = 0; i < VW; ++i) {
      const float d = q.e[i] - tgt[j + i];
      acc += d * d;
    }
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) row_loss[blockIdx.x] = acc / (float)K;
}

// loss[0] = (sum_i row_loss[i]) / count: thread t adds rows t, t + 256, ... in ascending order, then block_sum (fixed order).
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_mean_kernel(const float* __restrict__ row_loss, int64_t n, float count,
                                                                    float* __restrict__ loss) {
  __shared__ float red[16];
  const float a = block_strided_sum(row_loss, n, red);
  if (threadIdx.x == 0) loss[0] = a / count;
}

// One workgroup per row of dpred [V][lead + L][3 p^2]: scale * (pred - target) on a removed patch, exactly 0 on a kept patch and on the
// `lead` rows.  scale = gscale * 2 / (3 p^2 * V * (L - Lk)).
template <int DT, int DTO, int VW>
__global__ __launch_bounds__(MAE_THREADS) void mae_loss_bwd_kernel(const void* __restrict__ pred, const float* __restrict__ x,
                                                                   const int* __restrict__ ids_restore, void* __restrict__ dpred, int H,
                                                                   int W, int p, int Lk, int lead, float scale) {
  __shared__ float tgt[3 * MAE_MAX_PATCH * MAE_MAX_PATCH];
  const int L = (W / p) * (H / p), K = 3 * p * p, rows = lead + L;
  const int64_t v = blockIdx.x / rows;
  const int row = blockIdx.x % rows, l = row - lead;
  const int64_t base = (int64_t)blockIdx.x * K;
  int r = 0;
  if (l >= 0) r = ids_restore[v * L + l];
  if (l < 0 || (r >= 0 && r < Lk)) {                      // (uniform over the workgroup)
    const fvec<VW> z = vzero<VW>();
    for (int j = threadIdx.x * VW; j < K; j += MAE_THREADS * VW) st_dt<DTO, VW>(dpred, base + j, z);
    return;
  }
  mae_stage_target(x, tgt, v, l, H, W, p);
  for (int j = threadIdx.x * VW; j < K; j += MAE_THREADS * VW) {
    fvec<VW> q = ld_dt<DT, VW>(pred, base + j);
#pragma unroll
    for (int i = 0; i < VW; ++i) q.e[i] = scale * (q.e[i] - tgt[j + i]);
    st_dt<DTO, VW>(dpred, base + j, q);
  }
}

template <int DT, int DTO>
static void mae_loss_bwd_vw(bool vec, dim3 grid, hipStream_t st, const void* pred, const float* x, const int* ids_restore, void* dpred, int H,
                            int W, int p, int Lk, int lead, float scale) {
  if (vec) hipLaunchKernelGGL((mae_loss_bwd_kernel<DT, DTO, 4>), grid, dim3(MAE_THREADS), 0, st, pred, x, ids_restore, dpred, H, W, p, Lk, lead, scale);
  else hipLaunchKernelGGL((mae_loss_bwd_kernel<DT, DTO, 1>), grid, dim3(MAE_THREADS), 0, st, pred, x, ids_restore, dpred, H, W, p, Lk, lead, scale);
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// V samples of L patches of which 1 <= Lk < L are kept; D features.  (V * (1 + L) rows index a 32-bit grid in the loss kernels.)
static bool mae_shape_ok(int V, int L, int Lk, int D) {
  return V >= 1 && V <= (1 << 20) && L >= 2 && L <= MAE_MAX_L && Lk >= 1 && Lk < L && D >= 1 && D <= (1 << 16) &&
         (int64_t)V * (1 + L) <= 0x7fffffff;
}
static bool mae_image_ok(int V, int H, int W, int patch, int Lk) {
  if (!(H > 0 && W > 0 && patch > 0 && H % patch == 0 && W % patch == 0 && H <= (1 << 14) && W <= (1 << 14))) return false;
  const int64_t L = (int64_t)(H / patch) * (W / patch);
  return L <= MAE_MAX_L && mae_shape_ok(V, (int)L, Lk, 1);
}

extern "C" int dinox_mae_mask_ids(const float* noise, int* ids_restore, int* ids_keep, int V, int L, int Lk, void* stream) {
  DX_REQUIRE(noise && ids_restore && ids_keep, DINOX_EINVAL, "mae_mask_ids: null pointer");
  DX_REQUIRE(mae_shape_ok(V, L, Lk, 1), DINOX_EINVAL, "mae_mask_ids: V=%d L=%d Lk=%d (V >= 1, 2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, MAE_MAX_L);
  hipLaunchKernelGGL(mae_mask_ids_kernel, dim3((unsigned)V), dim3(MAE_THREADS), 0, as_stream(stream), noise, ids_restore, ids_keep, L, Lk);
  return check_launch("mae_mask_ids");
}

extern "C" int dinox_mae_gather_unfold(const float* x, const int* ids_keep, void* u, int V, int H, int W, int patch, int Lk, int ld,
                                       int out_dtype, void* stream) {
  DX_REQUIRE(x && ids_keep && u, DINOX_EINVAL, "mae_gather_unfold: null pointer");
  DX_REQUIRE(dtype_ok(out_dtype), DINOX_EINVAL, "mae_gather_unfold: dtype %d", out_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= 1024 && ld >= 3 * patch * patch && ld <= (1 << 22), DINOX_EINVAL,
             "mae_gather_unfold: V=%d H=%d W=%d patch=%d Lk=%d ld=%d (H, W multiples of patch; 2 <= L <= %d; 1 <= Lk < L; ld >= 3 patch^2)", V, H,
             W, patch, Lk, ld, MAE_MAX_L);
  const bool vec = patch % 4 == 0 && ld % 4 == 0 && aligned16(x, u);
  const dim3 grid(grid_1d((int64_t)V * Lk * (ld / (vec ? 4 : 1)), MAE_THREADS, 4096));
  DX_LAUNCH_DT_VW(mae_gather_unfold_kernel, out_dtype, vec, grid, dim3(MAE_THREADS), as_stream(stream), x, ids_keep, u, V, H, W, patch, Lk, ld);
  return check_launch("mae_gather_unfold");
}

extern "C" int dinox_mae_tokens_fwd(const void* patches, const float* cls, const float* pos, const int* ids_keep, float* tokens, int V, int L,
                                    int Lk, int D, int patches_dtype, void* stream) {
  DX_REQUIRE(patches && cls && pos && ids_keep && tokens, DINOX_EINVAL, "mae_tokens_fwd: null pointer");
  DX_REQUIRE(dtype_ok(patches_dtype), DINOX_EINVAL, "mae_tokens_fwd: dtype %d", patches_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_tokens_fwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, MAE_MAX_L);
  const bool vec = D % 4 == 0 && aligned16(patches, cls, pos, tokens);
  const dim3 grid(grid_1d((int64_t)V * (1 + Lk) * (D / (vec ? 4 : 1)), MAE_THREADS, 4096));
  DX_LAUNCH_DT_VW(mae_tokens_fwd_kernel, patches_dtype, vec, grid, dim3(MAE_THREADS), as_stream(stream), patches, cls, pos, ids_keep, tokens, V, L, Lk, D);
  return check_launch("mae_tokens_fwd");
}

extern "C" int dinox_mae_tokens_bwd(const float* dtokens, const int* ids_restore, void* dpatches, float* dcls, float* dpos, int V, int L, int Lk,
                                    int D, int patches_dtype, void* stream) {
  DX_REQUIRE(dtokens && ids_restore && dpatches && dcls && dpos, DINOX_EINVAL, "mae_tokens_bwd: null pointer");
  DX_REQUIRE(dtype_ok(patches_dtype), DINOX_EINVAL, "mae_tokens_bwd: dtype %d", patches_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_tokens_bwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, MAE_MAX_L);
  const bool vec = D % 4 == 0 && aligned16(dtokens, dpatches, dcls, dpos);
  const int DV = D / (vec ? 4 : 1), chunks = (int)ceil_div(DV, MAE_THREADS), param_blocks = (1 + L) * chunks;
  const dim3 grid((unsigned)param_blocks + grid_1d((int64_t)V * Lk * DV, MAE_THREADS, 4096));
  DX_LAUNCH_DT_VW(mae_tokens_bwd_kernel, patches_dtype, vec, grid, dim3(MAE_THREADS), as_stream(stream), dtokens, ids_restore, dpatches, dcls, dpos, V, L,
                  Lk, D, chunks, param_blocks);
  return check_launch("mae_tokens_bwd");
}

extern "C" int dinox_mae_unshuffle_fwd(const void* e, const float* mask_token, const float* dec_pos, const int* ids_restore, float* xd, int V,
                                       int L, int Lk, int D, int e_dtype, void* stream) {
  DX_REQUIRE(e && mask_token && dec_pos && ids_restore && xd, DINOX_EINVAL, "mae_unshuffle_fwd: null pointer");
  DX_REQUIRE(dtype_ok(e_dtype), DINOX_EINVAL, "mae_unshuffle_fwd: dtype %d", e_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_unshuffle_fwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, MAE_MAX_L);
  const bool vec = D % 4 == 0 && aligned16(e, mask_token, dec_pos, xd);
  const dim3 grid(grid_1d((int64_t)V * (1 + L) * (D / (vec ? 4 : 1)), MAE_THREADS, 4096));
  DX_LAUNCH_DT_VW(mae_unshuffle_fwd_kernel, e_dtype, vec, grid, dim3(MAE_THREADS), as_stream(stream), e, mask_token, dec_pos, ids_restore, xd, V, L, Lk, D);
  return check_launch("mae_unshuffle_fwd");
}

extern "C" int dinox_mae_unshuffle_bwd(const float* g, const int* ids_keep, const int* ids_restore, void* de, float* dmask_token, float* ws,
                                       int V, int L, int Lk, int D, int de_dtype, void* stream) {
  DX_REQUIRE(g && ids_keep && ids_restore && de && dmask_token && ws, DINOX_EINVAL, "mae_unshuffle_bwd: null pointer");
  DX_REQUIRE(dtype_ok(de_dtype), DINOX_EINVAL, "mae_unshuffle_bwd: dtype %d", de_dtype);
  DX_REQUIRE(mae_shape_ok(V, L, Lk, D), DINOX_EINVAL, "mae_unshuffle_bwd: V=%d L=%d Lk=%d D=%d (2 <= L <= %d, 1 <= Lk < L)", V, L, Lk, D, MAE_MAX_L);
  hipStream_t st = as_stream(stream);
  const bool vec = D % 4 == 0 && aligned16(g, de, dmask_token, ws);
  const int DV = D / (vec ? 4 : 1), chunks = (int)ceil_div(DV, MAE_THREADS), part_blocks = V * chunks;
  const dim3 grid((unsigned)part_blocks + grid_1d((int64_t)V * (1 + Lk) * DV, MAE_THREADS, 4096));
  DX_LAUNCH_DT_VW(mae_unshuffle_bwd_kernel, de_dtype, vec, grid, dim3(MAE_THREADS), st, g, ids_keep, ids_restore, de, ws, V, L, Lk, D, chunks, part_blocks);
  int rc = check_launch("mae_unshuffle_bwd");
  if (rc) return rc;
  if (vec) hipLaunchKernelGGL(mae_colsum_rows_kernel<4>, dim3((unsigned)chunks), dim3(MAE_THREADS), 0, st, ws, dmask_token, V, D);
  else hipLaunchKernelGGL(mae_colsum_rows_kernel<1>, dim3((unsigned)chunks), dim3(MAE_THREADS), 0, st, ws, dmask_token, V, D);
  return check_launch("mae_unshuffle_bwd_mask");
}

extern "C" int dinox_mae_loss_fwd(const void* pred, const float* x, const int* ids_restore, float* loss, float* ws, int V, int H, int W, int patch,
                                  int Lk, int lead, int pred_dtype, void* stream) {
  DX_REQUIRE(pred && x && ids_restore && loss && ws, DINOX_EINVAL, "mae_loss_fwd: null pointer");
  DX_REQUIRE(dtype_ok(pred_dtype), DINOX_EINVAL, "mae_loss_fwd: dtype %d", pred_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= MAE_MAX_PATCH && (lead == 0 || lead == 1), DINOX_EINVAL,
             "mae_loss_fwd: V=%d H=%d W=%d patch=%d Lk=%d lead=%d (H, W multiples of patch <= %d; 2 <= L <= %d; 1 <= Lk < L; lead 0 or 1)", V, H, W,
             patch, Lk, lead, MAE_MAX_PATCH, MAE_MAX_L);
  hipStream_t st = as_stream(stream);
  const int L = (H / patch) * (W / patch), K = 3 * patch * patch;
  const bool vec = K % 4 == 0 && aligned16(pred);
  const dim3 grid((unsigned)((int64_t)V * L));
  DX_LAUNCH_DT_VW(mae_loss_rows_kernel, pred_dtype, vec, grid, dim3(MAE_THREADS), st, pred, x, ids_restore, ws, H, W, patch, Lk, lead);
  int rc = check_launch("mae_loss_fwd");
  if (rc) return rc;
  hipLaunchKernelGGL(mae_loss_mean_kernel, dim3(1), dim3(MAE_THREADS), 0, st, ws, (int64_t)V * L, (float)V * (float)(L - Lk), loss);
  return check_launch("mae_loss_fwd_mean");
}

extern "C" int dinox_mae_loss_bwd(const void* pred, const float* x, const int* ids_restore, void* dpred, float gscale, int V, int H, int W,
                                  int patch, int Lk, int lead, int pred_dtype, int dpred_dtype, void* stream) {
  DX_REQUIRE(pred && x && ids_restore && dpred, DINOX_EINVAL, "mae_loss_bwd: null pointer");
  DX_REQUIRE(dtype_ok(pred_dtype) && dtype_ok(dpred_dtype), DINOX_EINVAL, "mae_loss_bwd: dtypes %d, %d", pred_dtype, dpred_dtype);
  DX_REQUIRE(mae_image_ok(V, H, W, patch, Lk) && patch <= MAE_MAX_PATCH && (lead == 0 || lead == 1), DINOX_EINVAL,
             "mae_loss_bwd: V=%d H=%d W=%d patch=%d Lk=%d lead=%d (H, W multiples of patch <= %d; 2 <= L <= %d; 1 <= Lk < L; lead 0 or 1)", V, H, W,
             patch, Lk, lead, MAE_MAX_PATCH, MAE_MAX_L);
  DX_REQUIRE(dpred != pred, DINOX_EINVAL, "mae_loss_bwd: dpred must not alias pred");
  hipStream_t st = as_stream(stream);
  const int L = (H / patch) * (W / patch), K = 3 * patch * patch;
  const bool vec = K % 4 == 0 && aligned16(pred, dpred);
  const dim3 grid((unsigned)((int64_t)V * (lead + L)));
  const float scale = (float)((double)gscale * 2.0 / ((double)K * (double)V * (double)(L - Lk)));
  if (pred_dtype == DINOX_F32 && dpred_dtype == DINOX_F32) mae_loss_bwd_vw<DINOX_F32, DINOX_F32>(vec, grid, st, pred, x, ids_restore, dpred, H, W, patch, Lk, lead, scale);
  else if (pred_dtype == DINOX_F32) mae_loss_bwd_vw<DINOX_F32, DINOX_BF16>(vec, grid, st, pred, x, ids_restore, dpred, H, W, patch, Lk, lead, scale);
  else if (dpred_dtype == DINOX_F32) mae_loss_bwd_vw<DINOX_BF16, DINOX_F32>(vec, grid, st, pred, x, ids_restore, dpred, H, W, patch, Lk, lead, scale);
  else mae_loss_bwd_vw<DINOX_BF16, DINOX_BF16>(vec, grid, st, pred, x, ids_restore, dpred, H, W, patch, Lk, lead, scale);
  return check_launch("mae_loss_bwd");
}
