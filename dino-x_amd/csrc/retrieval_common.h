// retrieval_common.h -- what the similarity sweeps share (retrieval.hip: rank of the positive; knn.hip: the K nearest keys): the tile shape,
// the key-split policy, the staging of 128 rows x 16 k through LDS and the MFMA loop of one 128 keys x 128 queries tile.  Both files run the
// SAME instruction sequence per score (exact-fp32 MFMA, d-ordered fma chain, keys on the row side), so a score is bitwise the same in both.
#pragma once
#include "common.h"

namespace dinox {

constexpr int RR_TQ = 128, RR_TK = 128, RR_BK = 16, RR_THREADS = 256;
constexpr int RR_LD = RR_TK + 4;               // LDS row pitch (floats): the four k-quads of a staging store land 16 banks apart
// Key splits, a pure function of (Nq, Nk) so that dinox_retrieval_ws_bytes and the launch always agree (measured on MI355X,
// tools/retrieval_bench.py, DESIGN.md "Retrieval"): the sweep holds three workgroups per CU, 768 on the
// chip.  Many small workgroups balance the tail of a long sweep (N = 16 384: 2048 workgroups of 8 tiles beat 1024 of 16 by 7 %); but a grid
// just above 768 one-tile workgroups ends with one workgroup per CU and nothing to hide its barriers behind (N = 4096: 1024 x 1 tile
// 204 us, 512 x 2 tiles 177 us), so a grid that cannot be resident at once gives every workgroup at least two tiles.
constexpr int64_t RR_TARGET_GROUPS = 2048, RR_RESIDENT_GROUPS = 768;

struct RrSplit {
  int64_t strips, tiles_per_split, splits;
};

static RrSplit rr_split(int64_t Nq, int64_t Nk) {
  RrSplit s;
  s.strips = ceil_div(Nq, (int64_t)RR_TQ);
  const int64_t tiles = ceil_div(Nk, (int64_t)RR_TK);
  int64_t want = ceil_div(RR_TARGET_GROUPS, s.strips);
  if (want > tiles) want = tiles;
  if (want > 65535) want = 65535;              // grid.y
  s.tiles_per_split = ceil_div(tiles, want);
  if (s.tiles_per_split < 2 && tiles >= 2 && s.strips * tiles > RR_RESIDENT_GROUPS) s.tiles_per_split = 2;
  s.splits = ceil_div(tiles, s.tiles_per_split);   // no empty split
  return s;
}

// (value, index) maximum with the lowest index on equal values
__device__ __forceinline__ void rr_max(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// 128 rows x 16 k of a row-major operand: 512 quads, two per thread; four neighbouring threads read 64 contiguous bytes of a row.
// VEC: every quad is 16-byte aligned and whole (pointer, leading dimension and D multiples of four floats) -- one dwordx4 load per quad;
// otherwise element loads.  Rows past the end and k past D read as zero (no load is issued for them).
template <bool VEC>
__device__ __forceinline__ void rr_fetch(const float* __restrict__ base, int64_t ld, int64_t row0, int64_t rows, int64_t k0, int64_t D,
                                         f32x4 (&v)[2]) {
  const int t = threadIdx.x;
  const int64_t gk = k0 + 4 * (t & 3);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t gr = row0 + (t >> 2) + 64 * i;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (gr < rows) {
      const float* p = base + gr * ld + gk;
      if constexpr (VEC) {
        if (gk < D) x = *reinterpret_cast<const f32x4*>(p);
      } else {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (gk + cc < D) x[cc] = p[cc];
      }
    }
    v[i] = x;
  }
}

__device__ __forceinline__ void rr_put(const f32x4 (&v)[2], float (*dst)[RR_LD]) {
  const int t = threadIdx.x, kq = 4 * (t & 3);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) dst[kq + cc][(t >> 2) + 64 * i] = v[i][cc];
}

// One tile: acc[i][j][e] = s(query q0 + wc 64 + j 32 + c, key k0row + wr 64 + i 32 + (e & 3) + 8 (e >> 2) + 4 h) with c = lane & 31,
// h = lane >> 5, wr = wave >> 1 (which 64 keys of the tile), wc = wave & 1 (which 64 queries of the strip).  Keys past Nk and queries past
// Nq are multiplied as zero rows.  Ends on a barrier: Ks / Qs are free again.
template <bool VEC>
__device__ __forceinline__ void rr_tile(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk, int64_t q0,
                                        int64_t Nq, int64_t k0row, int64_t Nk, int64_t D, float (*Ks)[RR_LD], float (*Qs)[RR_LD],
                                        f32x16 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  f32x4 vk[2], vq[2];
  rr_fetch<VEC>(k, ldk, k0row, Nk, 0, D, vk);
  rr_fetch<VEC>(q, ldq, q0, Nq, 0, D, vq);
  for (int64_t d0 = 0; d0 < D; d0 += RR_BK) {
    rr_put(vk, Ks);
    rr_put(vq, Qs);
    __syncthreads();
    if (d0 + RR_BK < D) {                                  // next slab: in flight under the products below
      rr_fetch<VEC>(k, ldk, k0row, Nk, d0 + RR_BK, D, vk);
      rr_fetch<VEC>(q, ldq, q0, Nq, d0 + RR_BK, D, vq);
    }
#pragma unroll
    for (int kk = 0; kk < RR_BK; kk += 2) {
      const int kr = kk + h;
      const float a0 = Ks[kr][wr * 64 + c], a1 = Ks[kr][wr * 64 + 32 + c];
      const float b0 = Qs[kr][wc * 64 + c], b1 = Qs[kr][wc * 64 + 32 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
}

}  // namespace dinox
