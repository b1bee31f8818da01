// labelprop.hip -- one step of dense label propagation (Caron et al. 2021, the video-segmentation protocol of DINO, with the z axis of a CT
// series as the sequence): for every patch of the target slice the K best-matching patches of F context slices inside a spatial window,
// then a softmax-weighted vote over their soft labels.  In torch this is an [N, F N] affinity matrix, a mask, a topk and a matmul per
// slice; here the matrix never exists (the sweep of knn.hip) and the window removes whole key tiles.
//
//   queries   q [N][D], N = g g, patch p = y g + x          keys   k [F N][D], key j = f N + y' g + x'          seg [F N][C]
//   candidates of p:  the keys with |y' - y| <= R and |x' - x| <= R  (R = radius; radius < 0 or >= g - 1: the whole grid), in every slot f
//   s(p, j) = sum_d q[p,d] k[j,d]     the tile loop of retrieval_common.h: a score is bitwise the score dinox_knn_topk sees
//   selection:  the first K candidates in the order (score descending, key index ascending) -- knn_before, knn_common.h
//   vote:  w_i = exp((s_i - s_1) inv_temperature) over the filled slots,  out[p][c] = sum_i w_i seg[j_i][c] / sum_i w_i
//
// Two launches on the caller's stream:
//   1. labelprop_sweep:   grid = (query strips, key splits), the sweep of knn_sweep with two additions.  A key tile is SKIPPED (no load, no
//      product) when no key of it lies in a grid row within R of a grid row of the strip's queries: a strip is 128 consecutive patches,
//      i.e. whole grid rows but for its ends, so the row band is the window of the strip up to those ends; the test is three divisions by
//      g per tile, uniform over the workgroup.  The band only ever lets through MORE than the windows do.  The window itself is tested on
//      the selection side, per (query, key) pair that passed the threshold compare: the (y', x') of the tile's 128 keys are put into LDS
//      once per tile, the lane holds the (y, x) of its two queries.
//   2. labelprop_finish:  one thread per query merges the splits' lists in ascending split order (knn_finish), then the vote.
//
// LDS of the sweep: the two 16 x 132 staging slabs 16.5 KiB, the lists [128][33] of (score, index) 33 KiB, the tile's key coordinates
// 0.5 KiB: 50 KiB, three workgroups on a CU's 160 KiB -- the occupancy knn_sweep runs at, which its __launch_bounds__ asks for.  The vote
// is not in the sweep's tail: with key splits a strip's lists are final only after the merge, and a vote there would add C <= 64 columns
// of accumulators to a kernel that sits at its register limit for three workgroups.
//
// Vote arithmetic (the bound of tests/_labelprop_oracle.py rests on it): the exponent argument is formed in double and rounded to fp32 once;
// expf is the precise one (1 ulp); the numerator is one fp32 fma chain over i ascending (K roundings); the denominator is summed over i
// ascending in fp32 with the rounding error of every addition carried along (TwoSum) and added once at the end, so it is rounded once; one division.
// Plain stores only, fixed merge order: two runs give identical bits.  A NaN score never enters a list.
#include "knn_common.h"

namespace dinox {

constexpr int LP_CMIN = 2, LP_CMAX = 64;

// does a key of [key_lo, key_hi] lie in a grid row of [ylo, yhi]?  Keys run row by row through the F slots: global row rho = key / g,
// grid row rho % g.
__device__ __forceinline__ bool lp_band_hit(int64_t key_lo, int64_t key_hi, int g, int ylo, int yhi) {
  const int64_t ra = key_lo / g, rb = key_hi / g;
  const int ya = (int)(ra % g);
  const int64_t first = ya <= yhi ? ra + (ya < ylo ? ylo - ya : 0) : ra + (g - ya) + ylo;      // the first row >= ra whose grid row is in the band
  return first <= rb;
}

// ------------------------------------------------------------------------------------------ 1. sweep
template <bool VEC>
__global__ __launch_bounds__(RR_THREADS, 3) void labelprop_sweep(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                                 int g, int R, int64_t Nq, int64_t Nk, int64_t D, int K, int64_t tiles_per_split,
                                                                 float* __restrict__ ws_val, int32_t* __restrict__ ws_idx) {
  __shared__ float Ks[RR_BK][RR_LD];
  __shared__ float Qs[RR_BK][RR_LD];
  __shared__ float lv[RR_TQ][KNN_LP];
  __shared__ int li[RR_TQ][KNN_LP];
  __shared__ unsigned kyx[RR_TK];                 // y' << 16 | x' of the tile's keys (g < 2^16 since F N < 2^31)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;           // wr: which 64 keys of the tile, wc: which 64 queries of the strip
  const int turn = 2 * wr + h;                   // the four holders of a query's keys write its list one after the other
  const int64_t q0 = (int64_t)blockIdx.x * RR_TQ;
  const int64_t tiles = ceil_div(Nk, (int64_t)RR_TK);
  const int64_t tile_lo = (int64_t)blockIdx.y * tiles_per_split;
  const int64_t tile_hi = tile_lo + tiles_per_split < tiles ? tile_lo + tiles_per_split : tiles;

  for (int t = threadIdx.x; t < RR_TQ * KNN_LP; t += RR_THREADS) {
    (&lv[0][0])[t] = -INFINITY;
    (&li[0][0])[t] = KNN_NONE;
  }
  // this lane's two queries (one per 32-wide column block) and where they sit in the grid
  int qy[2], qx[2];
  bool qok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qi = q0 + wc * 64 + j * 32 + c;
    qok[j] = qi < Nq;
    qy[j] = (int)(qi / g);
    qx[j] = (int)(qi - (int64_t)qy[j] * g);
  }
  // the grid rows within R of a row of the strip
  const int64_t q_last = q0 + RR_TQ < Nq ? q0 + RR_TQ - 1 : Nq - 1;
  const int y_first = (int)(q0 / g), y_last = (int)(q_last / g);
  const int ylo = y_first - R > 0 ? y_first - R : 0, yhi = y_last + R < g - 1 ? y_last + R : g - 1;
  __syncthreads();

  for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
    const int64_t k0row = tile * RR_TK;
    const int64_t k_last = k0row + RR_TK < Nk ? k0row + RR_TK - 1 : Nk - 1;
    if (!lp_band_hit(k0row, k_last, g, ylo, yhi)) continue;                     // uniform over the workgroup: no barrier is left out by some
    if (threadIdx.x < RR_TK) {                   // free since the last barrier of the previous tile; visible after the barriers of rr_tile (D >= 1)
      const int64_t key = k0row + threadIdx.x;
      const int64_t row = key / g;
      kyx[threadIdx.x] = (unsigned)(row % g) << 16 | (unsigned)(key - row * g);
    }
    f32x16 acc[2][2];
    rr_tile<VEC>(q, ldq, k, ldk, q0, Nq, k0row, Nk, D, Ks, Qs, acc);
    const int nk = (int)Nk, loc0 = wr * 64 + 4 * h, key0 = (int)k0row + loc0;
#pragma unroll 1
    for (int o = 0; o < 4; ++o) {
      if (o == turn) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float* rv = lv[wc * 64 + j * 32 + c];
          int* ri = li[wc * 64 + j * 32 + c];
          // the query's K-th best score in a register, as in knn_sweep: a score that cannot enter costs one v_cmp and no LDS access; the
          // window is looked up only for the survivors.  Queries past Nq take nothing.
          float thr = qok[j] ? rv[K - 1] : INFINITY;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int off = i * 32 + (e & 3) + 8 * (e >> 2);
              const int key = key0 + off;
              const float s = acc[i][j][e];
              if (s >= thr && key < nk) {
                const unsigned yx = kyx[loc0 + off];
                const int dy = (int)(yx >> 16) - qy[j], dx = (int)(yx & 0xffffu) - qx[j];
                if (dy <= R && -dy <= R && dx <= R && -dx <= R) {
                  knn_insert(rv, ri, K, s, key);
                  thr = rv[K - 1];
                }
              }
            }
        }
      }
      __syncthreads();
    }
  }

  for (int t = threadIdx.x; t < RR_TQ * K; t += RR_THREADS) {
    const int r = t / K, p = t - r * K;
    if (q0 + r < Nq) {
      const int64_t o = ((int64_t)blockIdx.y * Nq + q0 + r) * K + p;
      ws_val[o] = lv[r][p];
      ws_idx[o] = li[r][p];
    }
  }
}

// ------------------------------------------------------------------------------------------ 2. merge of the key splits, vote
__global__ __launch_bounds__(KNN_FIN_THREADS) void labelprop_finish(const float* __restrict__ ws_val, const int32_t* __restrict__ ws_idx,
                                                                    const float* __restrict__ seg, int64_t Nq, int splits, int K, int C,
                                                                    float inv_t, float* __restrict__ out, int32_t* __restrict__ out_idx,
                                                                    float* __restrict__ out_val) {
  __shared__ float lv[KNN_FIN_THREADS][KNN_LP];  // the merged scores, then the weights
  __shared__ int li[KNN_FIN_THREADS][KNN_LP];
  __shared__ float wsum[KNN_FIN_THREADS];
  const int64_t i0 = (int64_t)blockIdx.x * KNN_FIN_THREADS, i = i0 + threadIdx.x;
  if (i < Nq) {
    float* rv = lv[threadIdx.x];
    int* ri = li[threadIdx.x];
    for (int p = 0; p < K; ++p) {
      rv[p] = -INFINITY;
      ri[p] = KNN_NONE;
    }
    for (int s = 0; s < splits; ++s) {           // ascending split = ascending key range: a fixed order
      const int64_t o = ((int64_t)s * Nq + i) * K;
      for (int p = 0; p < K; ++p) {
        const float v = ws_val[o + p];
        const int ix = ws_idx[o + p];
        if (ix == KNN_NONE || !knn_before(v, ix, rv[K - 1], ri[K - 1])) break;      // the split's list is ordered: nothing after this enters
        knn_insert(rv, ri, K, v, ix);
      }
    }
    // weights of the filled slots (a prefix of the list); the sum keeps the rounding error of every addition (TwoSum) and adds it once
    const float s1 = rv[0];
    float sum = 0.f, err = 0.f;
    for (int p = 0; p < K; ++p) {
      const int ix = ri[p];
      const float v = rv[p];
      out_idx[i * K + p] = ix == KNN_NONE ? -1 : ix;
      out_val[i * K + p] = ix == KNN_NONE ? -INFINITY : v;
      float w = 0.f;
      if (ix != KNN_NONE) {
        w = expf((float)(((double)v - (double)s1) * (double)inv_t));
        const float t = sum + w, bv = t - sum;
        err += (sum - (t - bv)) + (w - bv);
        sum = t;
      }
      rv[p] = w;
    }
    wsum[threadIdx.x] = sum + err;
  }
  __syncthreads();
  const int rows = Nq - i0 < KNN_FIN_THREADS ? (int)(Nq - i0) : KNN_FIN_THREADS;
  for (int t = threadIdx.x; t < rows * C; t += KNN_FIN_THREADS) {   // consecutive threads: consecutive classes of a row of seg
    const int r = t / C, cc = t - r * C;
    float num = 0.f;
    bool any = false;
    for (int p = 0; p < K; ++p) {
      const int ix = li[r][p];
      if (ix == KNN_NONE) break;
      any = true;
      num = fmaf(lv[r][p], seg[(int64_t)ix * C + cc], num);
    }
    out[(i0 + r) * C + cc] = any ? num / wsum[r] : 0.f;
  }
}

// N = g g and F N within the int range the sweeps guard; 0 where not
static int64_t lp_keys(int g, int F) {
  if (g < 1 || F < 1) return 0;
  const int64_t N = (int64_t)g * g;
  if (N > 0x7fffffff - RR_TQ || (int64_t)F > (0x7fffffff - RR_TK) / N) return 0;
  return (int64_t)F * N;
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_labelprop_ws_bytes(int g, int F, int D, int C, int K) {
  const int64_t Nk = lp_keys(g, F);
  if (Nk == 0 || D < 1 || C < LP_CMIN || C > LP_CMAX || K < 1 || K > KNN_KMAX) return 0;   // what dinox_labelprop refuses
  const int64_t N = (int64_t)g * g;
  return knn_split(N, Nk).splits * N * K * 8;     // an ordered (score, index) list of K per query and key split
}

extern "C" int dinox_labelprop(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* seg, int g, int F, int D, int C, int K,
                               int radius, float inv_temperature, float* out, int32_t* out_idx, float* out_val, void* ws, void* stream) {
  DX_REQUIRE(K >= 1 && K <= KNN_KMAX, DINOX_EINVAL, "labelprop: K=%d outside [1, %d]", K, KNN_KMAX);
  DX_REQUIRE(C >= LP_CMIN && C <= LP_CMAX, DINOX_EINVAL, "labelprop: C=%d outside [%d, %d]", C, LP_CMIN, LP_CMAX);
  DX_REQUIRE(q && k && seg && out && out_idx && out_val && ws, DINOX_EINVAL, "labelprop: null pointer");
  DX_REQUIRE(g >= 1 && F >= 1 && D >= 1, DINOX_EINVAL, "labelprop: g=%d F=%d D=%d (each must be >= 1)", g, F, D);
  DX_REQUIRE(ldq >= D && ldk >= D, DINOX_EINVAL, "labelprop: ldq=%lld ldk=%lld below D=%d", (long long)ldq, (long long)ldk, D);
  DX_REQUIRE(inv_temperature > 0.f && inv_temperature <= 3.402823466e38f, DINOX_EINVAL, "labelprop: inv_temperature=%g must be finite and > 0",
             (double)inv_temperature);
  const int64_t Nk = lp_keys(g, F);
  DX_REQUIRE(Nk > 0, DINOX_EINVAL, "labelprop: g=%d F=%d: F g g keys exceed 2^31 - %d", g, F, RR_TK + 1);   // (padded indices of the last tile stay in int)
  const int64_t N = (int64_t)g * g;
  const int R = (radius < 0 || radius >= g - 1) ? g : radius;                  // g: every |dy|, |dx| <= g - 1 passes
  const RrSplit sp = knn_split(N, Nk);
  const bool vec = (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && D % 4 == 0;
  float* ws_val = (float*)ws;
  int32_t* ws_idx = (int32_t*)(ws_val + sp.splits * N * K);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)sp.strips, (unsigned)sp.splits);
#define LP_SWEEP(V) \
  hipLaunchKernelGGL(labelprop_sweep<V>, grid, dim3(RR_THREADS), 0, st, q, ldq, k, ldk, g, R, N, Nk, (int64_t)D, K, sp.tiles_per_split, ws_val, ws_idx)
  if (vec) LP_SWEEP(true); else LP_SWEEP(false);
#undef LP_SWEEP
  if (int rc = check_launch("labelprop_sweep")) return rc;
  hipLaunchKernelGGL(labelprop_finish, dim3((unsigned)ceil_div(N, (int64_t)KNN_FIN_THREADS)), dim3(KNN_FIN_THREADS), 0, st, (const float*)ws_val,
                     (const int32_t*)ws_idx, seg, N, (int)sp.splits, K, C, inv_temperature, out, out_idx, out_val);
  return check_launch("labelprop_finish");
}
