// retrieval.hip -- label-free view-retrieval score: per query, the RANK of its positive key in a similarity sweep, without ever
// holding the similarity matrix.  Replaces the host block of the reference's scripts/phase5_view_retrieval_eval.py:214-227
// (S = Q K^T as an N x N numpy array, argmax / argpartition over its rows: 64 MB at N = 4096, 17 GB at N = 65 536).
//
//   s(i,j)     = sum_d q[i,d] k[j,d]              exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): per score a d-ordered fp32 fma chain
//   pos_val[i] = s(i, target[i])
//   rank[i]    = #{j : s(i,j) > pos_val[i]} + #{j < target[i] : s(i,j) == pos_val[i]}      (place in a stable descending sort)
//   best_val[i], best_idx[i] = max_j s(i,j) and its lowest index                           (np.argmax: first maximum)
//
// Three launches on the caller's stream:
//   1. retrieval_pos:    pos_val.  A wave multiplies 32 key rows GATHERED by target against its 32 query rows on the same MFMA, in the
//                        same d order and with the same operand roles as the sweep, and keeps the diagonal: the value is bitwise the
//                        score the sweep finds in column target[i], which is what gives the tie term a meaning.
//   2. retrieval_sweep:  128 keys x 128 queries per tile, the loop structure of gemm_f32_big (gemm_f32.hip) with the KEYS on the MFMA's
//                        row side: a lane then owns one query per 32-wide column block and its 16 accumulators of a block are 16 keys,
//                        so the compare / count / running maximum of the epilogue needs five registers per query column instead of
//                        five per accumulator.  grid = (query strips, key splits); a workgroup walks the key tiles of its split
//                        and stores one (count, max, argmax) triple per query into the workspace.
//   3. retrieval_finish: one thread per query adds the counts and merges the maxima of the splits in ascending split order.
// Plain stores only, no atomics: two runs give identical bits.
//
// dinox_retrieval_rank_windowed is the same three launches with every "over j" restricted to a per-query key window
// [key_lo[i], key_hi[i]) -- the per-dataset view retrieval of the pan-organ evaluation, where the rows are sorted by dataset and a
// query competes with the keys of its own dataset only.  Its sweep (retrieval_sweep_windowed) walks, per query strip, only the key tiles
// some window of the strip touches; tiles start at multiples of RR_TK of the GLOBAL key index and go through the same rr_tile, so a
// score is bitwise the one the unwindowed sweep computes.  dinox_row_dots is launch 1 on its own.
#include "retrieval_common.h"

namespace dinox {

__device__ __forceinline__ int rr_target(const int32_t* __restrict__ target, int64_t i, int64_t Nk) {
  int64_t t = target ? (int64_t)target[i] : i;
  t = t < 0 ? 0 : (t >= Nk ? Nk - 1 : t);      // a bad index must not become a bad address (documented in dinox.h: the caller's contract)
  return (int)t;
}

// Window of query i, clamped into [0, Nk] (a bad bound must not become an address or a loop bound): first key and width; an empty or
// inverted window has width 0.  lo + wd <= Nk, so "key in window" is one unsigned compare and implies key < Nk.
__device__ __forceinline__ void rr_window(const int32_t* __restrict__ key_lo, const int32_t* __restrict__ key_hi, int64_t i, int64_t Nk,
                                          int& lo, int& wd) {
  int64_t a = key_lo[i], b = key_hi[i];
  a = a < 0 ? 0 : (a > Nk ? Nk : a);
  b = b < 0 ? 0 : (b > Nk ? Nk : b);
  lo = (int)a;
  wd = b > a ? (int)(b - a) : 0;
}

// ------------------------------------------------------------------------------------------ 1. pos_val
// One wave per 32 queries.  MFMA operands straight from global memory (this pass is 1/128 of the sweep's work per key tile):
// lane l feeds row (l & 31), k = k0 + 2 j + (l >> 5) of its key row (A side) and of its query row (B side).  The zero fill of a ragged
// D is harmless to the chain: fma(0, 0, c) = c.
__global__ __launch_bounds__(RR_THREADS) void retrieval_pos(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                           const int32_t* __restrict__ target, int64_t Nq, int64_t Nk, int64_t D,
                                                           float* __restrict__ pos_val) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
  const int64_t i = ((int64_t)blockIdx.x * (RR_THREADS / 64) + (threadIdx.x >> 6)) * 32 + c;
  const int64_t ic = i < Nq ? i : Nq - 1;      // clamped: lanes past the end compute a row nobody stores
  const float* qr = q + ic * ldq;
  const float* kr = k + (int64_t)rr_target(target, ic, Nk) * ldk;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float a[RR_BK / 2], b[RR_BK / 2], an[RR_BK / 2], bn[RR_BK / 2];
  auto fetch = [&](int64_t k0, float (&x)[RR_BK / 2], float (&y)[RR_BK / 2]) {
#pragma unroll
    for (int j = 0; j < RR_BK / 2; ++j) {
      const int64_t kk = k0 + 2 * j + h;
      const bool ok = kk < D;
      x[j] = ok ? kr[kk] : 0.f;
      y[j] = ok ? qr[kk] : 0.f;
    }
  };
  fetch(0, an, bn);
  for (int64_t k0 = 0; k0 < D; k0 += RR_BK) {
#pragma unroll
    for (int j = 0; j < RR_BK / 2; ++j) {
      a[j] = an[j];
      b[j] = bn[j];
    }
    if (k0 + RR_BK < D) fetch(k0 + RR_BK, an, bn);           // next slab: in flight under the products below
#pragma unroll
    for (int j = 0; j < RR_BK / 2; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
  }
  // C(row r, column c) sits in lane (c, h) at register e with r = (e & 3) + 8 (e >> 2) + 4 h: the diagonal r = c
  const int e_diag = (c & 3) + 4 * (c >> 3);
  float v = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (e == e_diag) v = acc[e];
  if (h == ((c >> 2) & 1) && i < Nq) pos_val[i] = v;
}

// ------------------------------------------------------------------------------------------ 2. sweep
// (staging and the MFMA loop of one tile: rr_fetch / rr_put / rr_tile of retrieval_common.h, shared with knn.hip)
template <bool VEC>
__global__ __launch_bounds__(RR_THREADS, 3) void retrieval_sweep(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                             const int32_t* __restrict__ target, int64_t Nq, int64_t Nk, int64_t D,
                                                             const float* __restrict__ pos_val, int64_t tiles_per_split,
                                                             int32_t* __restrict__ ws_cnt, float* __restrict__ ws_val,
                                                             int32_t* __restrict__ ws_idx) {
  __shared__ float Ks[RR_BK][RR_LD];
  __shared__ float Qs[RR_BK][RR_LD];
  __shared__ int red_cnt[2][RR_TQ];
  __shared__ float red_val[2][RR_TQ];
  __shared__ int red_idx[2][RR_TQ];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;           // wr: which 64 keys of the tile, wc: which 64 queries of the strip
  const int64_t q0 = (int64_t)blockIdx.x * RR_TQ;
  const int64_t tiles = ceil_div(Nk, (int64_t)RR_TK);
  const int64_t tile_lo = (int64_t)blockIdx.y * tiles_per_split;
  const int64_t tile_hi = tile_lo + tiles_per_split < tiles ? tile_lo + tiles_per_split : tiles;

  // this lane's two queries (one per 32-wide column block), their positive score and positive index
  float pos[2], bv[2];
  int tgt[2], bi[2], cnt[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qi = q0 + wc * 64 + j * 32 + c;
    const bool ok = qi < Nq;
    pos[j] = ok ? pos_val[qi] : 0.f;
    tgt[j] = ok ? rr_target(target, qi, Nk) : 0;
    bv[j] = -INFINITY;
    bi[j] = 0x7fffffff;
    cnt[j] = 0;
  }

  for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
    const int64_t k0row = tile * RR_TK;
    f32x16 acc[2][2];
    rr_tile<VEC>(q, ldq, k, ldk, q0, Nq, k0row, Nk, D, Ks, Qs, acc);
    // epilogue on the accumulators: acc[i][j][e] = s(query j-block column c, key k0row + wr 64 + i 32 + (e & 3) + 8 (e >> 2) + 4 h).
    // Keys past Nk were multiplied as zero rows: they are neither counted nor allowed to win the maximum.
    const int nk = (int)Nk, key0 = (int)k0row + wr * 64 + 4 * h;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        __builtin_amdgcn_sched_barrier(0);                   // one 32 x 32 block at a time: 16 accumulator reads live, not 64
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = key0 + i * 32 + (e & 3) + 8 * (e >> 2);
          const float s = acc[i][j][e];
          if (key < nk) {
            cnt[j] += (s > pos[j] || (s == pos[j] && key < tgt[j])) ? 1 : 0;
            rr_max(bv[j], bi[j], s, key);
          }
        }
      }
  }

  // the two half-waves hold different keys of the same query; then the two key-side waves meet in LDS
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    cnt[j] += __shfl_xor(cnt[j], 32, 64);
    const float ov = __shfl_xor(bv[j], 32, 64);
    const int oi = __shfl_xor(bi[j], 32, 64);
    rr_max(bv[j], bi[j], ov, oi);
    if (h == 0) {
      const int col = wc * 64 + j * 32 + c;
      red_cnt[wr][col] = cnt[j];
      red_val[wr][col] = bv[j];
      red_idx[wr][col] = bi[j];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < RR_TQ && q0 + t < Nq) {
    float v = red_val[0][t];
    int ix = red_idx[0][t];
    rr_max(v, ix, red_val[1][t], red_idx[1][t]);
    const int64_t o = (int64_t)blockIdx.y * Nq + q0 + t;
    ws_cnt[o] = red_cnt[0][t] + red_cnt[1][t];
    ws_val[o] = v;
    ws_idx[o] = ix;
  }
}

// ------------------------------------------------------------------------------------------ 2w. windowed sweep
// The sweep above with a window per query.  grid = (query strips, key splits).  A workgroup reduces the windows of its 128 queries to
// their hull [ulo, uhi), walks the hull's key tiles tile_lo + blockIdx.y, + splits, ... (interleaved: the hull is a few tiles long and
// differs per strip, so contiguous ranges would leave most splits empty) and skips a tile no window of the strip touches -- a
// workgroup-uniform branch, the tile loop itself stays the straight-line rr_tile.  With rows sorted by group the work is
// sum n_g^2 scores, not Nq Nk.  The window test replaces the key < nk test of the unwindowed epilogue (it implies it): two more
// registers per query column (lo, width).
template <bool VEC>
__global__ __launch_bounds__(RR_THREADS, 3) void retrieval_sweep_windowed(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                                      int64_t ldk, const int32_t* __restrict__ target,
                                                                      const int32_t* __restrict__ key_lo, const int32_t* __restrict__ key_hi,
                                                                      int64_t Nq, int64_t Nk, int64_t D, const float* __restrict__ pos_val,
                                                                      int splits, int32_t* __restrict__ ws_cnt, float* __restrict__ ws_val,
                                                                      int32_t* __restrict__ ws_idx) {
  __shared__ float Ks[RR_BK][RR_LD];
  __shared__ float Qs[RR_BK][RR_LD];
  __shared__ int red_cnt[2][RR_TQ];
  __shared__ float red_val[2][RR_TQ];
  __shared__ int red_idx[2][RR_TQ];
  __shared__ int hull[2][RR_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int64_t q0 = (int64_t)blockIdx.x * RR_TQ;

  float pos[2], bv[2];
  int tgt[2], bi[2], cnt[2], lo[2], wd[2];
  int ulo = 0x7fffffff, uhi = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qi = q0 + wc * 64 + j * 32 + c;
    const bool ok = qi < Nq;
    pos[j] = ok ? pos_val[qi] : 0.f;
    tgt[j] = ok ? rr_target(target, qi, Nk) : 0;
    lo[j] = wd[j] = 0;                                       // queries past the end: an empty window
    if (ok) rr_window(key_lo, key_hi, qi, Nk, lo[j], wd[j]);
    bv[j] = -INFINITY;
    bi[j] = 0x7fffffff;
    cnt[j] = 0;
    if (wd[j] > 0) {
      ulo = lo[j] < ulo ? lo[j] : ulo;
      uhi = lo[j] + wd[j] > uhi ? lo[j] + wd[j] : uhi;
    }
  }
  // hull of the strip's windows: over the wave, then over the four waves (each query is held by two waves; min / max do not mind)
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int a = __shfl_xor(ulo, m, 64), b = __shfl_xor(uhi, m, 64);
    ulo = a < ulo ? a : ulo;
    uhi = b > uhi ? b : uhi;
  }
  if (lane == 0) {
    hull[0][wv] = ulo;
    hull[1][wv] = uhi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < RR_THREADS / 64; ++w) {
    ulo = hull[0][w] < ulo ? hull[0][w] : ulo;
    uhi = hull[1][w] > uhi ? hull[1][w] : uhi;
  }
  // 0 <= ulo < uhi <= Nk, or no window at all (uhi = 0: no tile)
  const int tile_hi = (uhi + RR_TK - 1) / RR_TK;

  for (int tile = ulo / RR_TK + (int)blockIdx.y; tile < tile_hi; tile += splits) {
    const int k0row = tile * RR_TK;
    const bool mine = (wd[0] > 0 && lo[0] < k0row + RR_TK && lo[0] + wd[0] > k0row) ||
                      (wd[1] > 0 && lo[1] < k0row + RR_TK && lo[1] + wd[1] > k0row);
    if (!__syncthreads_or(mine)) continue;                   // a gap of the hull: the same answer in every thread
    f32x16 acc[2][2];
    rr_tile<VEC>(q, ldq, k, ldk, q0, Nq, (int64_t)k0row, Nk, D, Ks, Qs, acc);
    // epilogue as in retrieval_sweep; a key counts for query column j only inside that query's window (which ends at or before Nk)
    const int key0 = k0row + wr * 64 + 4 * h;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = key0 + i * 32 + (e & 3) + 8 * (e >> 2);
          const float s = acc[i][j][e];
          if ((unsigned)(key - lo[j]) < (unsigned)wd[j]) {
            cnt[j] += (s > pos[j] || (s == pos[j] && key < tgt[j])) ? 1 : 0;
            rr_max(bv[j], bi[j], s, key);
          }
        }
      }
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    cnt[j] += __shfl_xor(cnt[j], 32, 64);
    const float ov = __shfl_xor(bv[j], 32, 64);
    const int oi = __shfl_xor(bi[j], 32, 64);
    rr_max(bv[j], bi[j], ov, oi);
    if (h == 0) {
      const int col = wc * 64 + j * 32 + c;
      red_cnt[wr][col] = cnt[j];
      red_val[wr][col] = bv[j];
      red_idx[wr][col] = bi[j];
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < RR_TQ && q0 + t < Nq) {
    float v = red_val[0][t];
    int ix = red_idx[0][t];
    rr_max(v, ix, red_val[1][t], red_idx[1][t]);
    const int64_t o = (int64_t)blockIdx.y * Nq + q0 + t;
    ws_cnt[o] = red_cnt[0][t] + red_cnt[1][t];
    ws_val[o] = v;
    ws_idx[o] = ix;
  }
}

// ------------------------------------------------------------------------------------------ 3. merge of the key splits
__global__ __launch_bounds__(RR_THREADS) void retrieval_finish(const int32_t* __restrict__ ws_cnt, const float* __restrict__ ws_val,
                                                              const int32_t* __restrict__ ws_idx, int64_t Nq, int splits,
                                                              int32_t* __restrict__ rank, int32_t* __restrict__ best_idx,
                                                              float* __restrict__ best_val) {
  const int64_t i = (int64_t)blockIdx.x * RR_THREADS + threadIdx.x;
  if (i >= Nq) return;
  int n = 0, bi = 0x7fffffff;
  float bv = -INFINITY;
  for (int s0 = 0; s0 < splits; s0 += 8) {        // ascending split = ascending key range: a fixed order; eight splits' loads in flight
    int c[8], ix[8];
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool ok = s0 + u < splits;
      const int64_t o = (int64_t)(ok ? s0 + u : s0) * Nq + i;
      c[u] = ok ? ws_cnt[o] : 0;
      v[u] = ok ? ws_val[o] : -INFINITY;
      ix[u] = ok ? ws_idx[o] : 0x7fffffff;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      n += c[u];
      rr_max(bv, bi, v[u], ix[u]);
    }
  }
  rank[i] = n;
  best_idx[i] = bi;
  best_val[i] = bv;
}

}  // namespace dinox

using namespace dinox;

// Key splits of the windowed sweep, a pure function of (Nq, Nk) like rr_split: a strip's hull is a few tiles long (a 512-row group
// spans 4 to 6), so up to four workgroups share it, fewer when the strips alone fill the chip's resident workgroups.
static int64_t rrw_splits(int64_t Nq, int64_t Nk) {
  const int64_t strips = ceil_div(Nq, (int64_t)RR_TQ), tiles = ceil_div(Nk, (int64_t)RR_TK);
  int64_t s = RR_RESIDENT_GROUPS / strips;
  if (s > 4) s = 4;
  if (s > tiles) s = tiles;
  return s < 1 ? 1 : s;
}

extern "C" int64_t dinox_retrieval_ws_bytes(int64_t Nq, int64_t Nk, int64_t D) {
  if (Nq <= 0 || Nk <= 0 || D <= 0 || Nq > 0x7fffffff - RR_TQ || Nk > 0x7fffffff - RR_TK) return 0;   // what the call refuses
  return rr_split(Nq, Nk).splits * Nq * 12;      // (count, maximum, its index) per query and key split
}

extern "C" int dinox_retrieval_rank(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* target, int64_t Nq, int64_t Nk,
                                    int64_t D, int32_t* rank, int32_t* best_idx, float* best_val, float* pos_val, void* ws, void* stream) {
  DX_REQUIRE(q && k && rank && best_idx && best_val && pos_val && ws, DINOX_EINVAL, "retrieval_rank: null pointer");
  DX_REQUIRE(Nq > 0 && Nk > 0 && D > 0 && Nq <= 0x7fffffff - RR_TQ && Nk <= 0x7fffffff - RR_TK && ldq >= D && ldk >= D, DINOX_EINVAL,   // (padded indices of the last tile stay in int)
             "retrieval_rank: Nq=%lld Nk=%lld D=%lld ldq=%lld ldk=%lld", (long long)Nq, (long long)Nk, (long long)D, (long long)ldq,
             (long long)ldk);
  DX_REQUIRE(target || Nq == Nk, DINOX_EINVAL, "retrieval_rank: a null target means target[i] = i and needs Nq == Nk (%lld, %lld)",
             (long long)Nq, (long long)Nk);
  const RrSplit sp = rr_split(Nq, Nk);
  DX_REQUIRE(sp.strips <= 0x7fffffff, DINOX_EINVAL, "retrieval_rank: Nq=%lld", (long long)Nq);
  const bool vec = (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && D % 4 == 0;
  int32_t* ws_cnt = (int32_t*)ws;
  float* ws_val = (float*)(ws_cnt + sp.splits * Nq);
  int32_t* ws_idx = (int32_t*)(ws_val + sp.splits * Nq);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(retrieval_pos, dim3((unsigned)ceil_div(Nq, (int64_t)(32 * RR_THREADS / 64))), dim3(RR_THREADS), 0, st, q, ldq, k, ldk,
                     target, Nq, Nk, D, pos_val);
  if (int rc = check_launch("retrieval_pos")) return rc;
  const dim3 grid((unsigned)sp.strips, (unsigned)sp.splits);
#define RR_SWEEP(V) \
  hipLaunchKernelGGL(retrieval_sweep<V>, grid, dim3(RR_THREADS), 0, st, q, ldq, k, ldk, target, Nq, Nk, D, (const float*)pos_val, \
                     sp.tiles_per_split, ws_cnt, ws_val, ws_idx)
  if (vec) RR_SWEEP(true); else RR_SWEEP(false);
#undef RR_SWEEP
  if (int rc = check_launch("retrieval_sweep")) return rc;
  hipLaunchKernelGGL(retrieval_finish, dim3((unsigned)ceil_div(Nq, (int64_t)RR_THREADS)), dim3(RR_THREADS), 0, st, (const int32_t*)ws_cnt,
                     (const float*)ws_val, (const int32_t*)ws_idx, Nq, (int)sp.splits, rank, best_idx, best_val);
  return check_launch("retrieval_finish");
}

extern "C" int64_t dinox_retrieval_rank_windowed_ws_bytes(int64_t Nq, int64_t Nk, int64_t D) {
  if (Nq <= 0 || Nk <= 0 || D <= 0 || Nq > 0x7fffffff - RR_TQ || Nk > 0x7fffffff - RR_TK) return 0;   // what the call refuses
  return rrw_splits(Nq, Nk) * Nq * 12;           // (count, maximum, its index) per query and key split
}

extern "C" int dinox_retrieval_rank_windowed(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* target,
                                             const int32_t* key_lo, const int32_t* key_hi, int64_t Nq, int64_t Nk, int64_t D, int32_t* rank,
                                             int32_t* best_idx, float* best_val, float* pos_val, void* ws, void* stream) {
  DX_REQUIRE(q && k && key_lo && key_hi && rank && best_idx && best_val && pos_val && ws, DINOX_EINVAL, "retrieval_rank_windowed: null pointer");
  DX_REQUIRE(Nq > 0 && Nk > 0 && D > 0 && Nq <= 0x7fffffff - RR_TQ && Nk <= 0x7fffffff - RR_TK && ldq >= D && ldk >= D, DINOX_EINVAL,
             "retrieval_rank_windowed: Nq=%lld Nk=%lld D=%lld ldq=%lld ldk=%lld", (long long)Nq, (long long)Nk, (long long)D, (long long)ldq,
             (long long)ldk);
  DX_REQUIRE(target || Nq == Nk, DINOX_EINVAL, "retrieval_rank_windowed: a null target means target[i] = i and needs Nq == Nk (%lld, %lld)",
             (long long)Nq, (long long)Nk);
  const int64_t strips = ceil_div(Nq, (int64_t)RR_TQ), splits = rrw_splits(Nq, Nk);
  DX_REQUIRE(strips <= 0x7fffffff, DINOX_EINVAL, "retrieval_rank_windowed: Nq=%lld", (long long)Nq);
  const bool vec = (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && D % 4 == 0;
  int32_t* ws_cnt = (int32_t*)ws;
  float* ws_val = (float*)(ws_cnt + splits * Nq);
  int32_t* ws_idx = (int32_t*)(ws_val + splits * Nq);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(retrieval_pos, dim3((unsigned)ceil_div(Nq, (int64_t)(32 * RR_THREADS / 64))), dim3(RR_THREADS), 0, st, q, ldq, k, ldk,
                     target, Nq, Nk, D, pos_val);
  if (int rc = check_launch("retrieval_pos")) return rc;
  const dim3 grid((unsigned)strips, (unsigned)splits);
#define RR_SWEEP(V) \
  hipLaunchKernelGGL(retrieval_sweep_windowed<V>, grid, dim3(RR_THREADS), 0, st, q, ldq, k, ldk, target, key_lo, key_hi, Nq, Nk, D, \
                     (const float*)pos_val, (int)splits, ws_cnt, ws_val, ws_idx)
  if (vec) RR_SWEEP(true); else RR_SWEEP(false);
#undef RR_SWEEP
  if (int rc = check_launch("retrieval_sweep_windowed")) return rc;
  hipLaunchKernelGGL(retrieval_finish, dim3((unsigned)ceil_div(Nq, (int64_t)RR_THREADS)), dim3(RR_THREADS), 0, st, (const int32_t*)ws_cnt,
                     (const float*)ws_val, (const int32_t*)ws_idx, Nq, (int)splits, rank, best_idx, best_val);
  return check_launch("retrieval_finish");
}

extern "C" int dinox_row_dots(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t N, int64_t D, float* out, void* stream) {
  DX_REQUIRE(a && b && out, DINOX_EINVAL, "row_dots: null pointer");
  DX_REQUIRE(N > 0 && D > 0 && N <= 0x7fffffff - RR_TQ && lda >= D && ldb >= D, DINOX_EINVAL, "row_dots: N=%lld D=%lld lda=%lld ldb=%lld",
             (long long)N, (long long)D, (long long)lda, (long long)ldb);
  // retrieval_pos with the roles of dinox_retrieval_rank(q = a, k = b, target = NULL): b on the MFMA's row side, a on its column side
  hipLaunchKernelGGL(retrieval_pos, dim3((unsigned)ceil_div(N, (int64_t)(32 * RR_THREADS / 64))), dim3(RR_THREADS), 0, as_stream(stream), a, lda,
                     b, ldb, (const int32_t*)nullptr, N, N, D, out);
  return check_launch("retrieval_pos");
}
