// knn.hip -- the K nearest keys of every query in a similarity sweep, without ever holding the similarity matrix.  Replaces the host block
// of the reference's scripts/evaluate_panorgan.py:526-529 (S = E E^T as an N x N numpy array, fill_diagonal(-inf), argpartition over its
// rows: 17 GB at N = 65 536) and feeds the weighted k-NN probe.
//
//   s(i,j) = sum_d q[i,d] k[j,d]     the tile loop of retrieval.hip (retrieval_common.h): exact-fp32 MFMA, d-ordered fma chain, keys on the
//                                    MFMA row side -- a score is bitwise the score dinox_retrieval_rank sees
//   row i of the output = the first K keys in the order (score descending, index ascending), key exclude[i] left out
//
// Selection: every query of a strip owns an ordered list of K (score, index) pairs in LDS ([128][K], 33 KB at the pitch used).  A lane owns
// one query per 32-wide column block; it compares each of its accumulators with a register copy of the query's K-th best score (one v_cmp per
// score, what the rank epilogue pays too; the copy is read inside the lane's own turn and refreshed after each insertion) and only the
// survivors walk into the list by insertion from the tail.  Four lanes hold keys of the
// same query (two half-waves x two key-side waves): they take turns, a barrier between the turns, so a list has one writer at a time and no
// atomic is needed.  The list is ordered by a total order, so the outcome does not depend on the order the keys arrive in.
// Two launches on the caller's stream:
//   1. knn_sweep:   grid = (query strips, key splits); a workgroup walks the key tiles of its split and stores its ordered K per query.
//   2. knn_finish:  one thread per query merges the splits' lists in ascending split order (each list is ordered: a split is left at its
//                   first entry that does not enter).
// Plain stores only: two runs give identical bits.  A NaN score compares false with everything and never enters a list.
#include "knn_common.h"

namespace dinox {

// ------------------------------------------------------------------------------------------ 1. sweep
template <bool VEC>
__global__ __launch_bounds__(RR_THREADS, 3) void knn_sweep(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k, int64_t ldk,
                                                           const int32_t* __restrict__ exclude, int64_t Nq, int64_t Nk, int64_t D, int K,
                                                           int64_t tiles_per_split, float* __restrict__ ws_val, int32_t* __restrict__ ws_idx) {
  __shared__ float Ks[RR_BK][RR_LD];
  __shared__ float Qs[RR_BK][RR_LD];
  __shared__ float lv[RR_TQ][KNN_LP];
  __shared__ int li[RR_TQ][KNN_LP];
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
  // this lane's two queries (one per 32-wide column block) and the key each of them leaves out
  int excl[2];
  bool qok[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int64_t qi = q0 + wc * 64 + j * 32 + c;
    qok[j] = qi < Nq;
    excl[j] = (qok[j] && exclude) ? exclude[qi] : -1;        // compared with key indices only: any value is safe, -1 matches none
  }
  __syncthreads();

  for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
    const int64_t k0row = tile * RR_TK;
    f32x16 acc[2][2];
    rr_tile<VEC>(q, ldq, k, ldk, q0, Nq, k0row, Nk, D, Ks, Qs, acc);
    const int nk = (int)Nk, key0 = (int)k0row + wr * 64 + 4 * h;
#pragma unroll 1
    for (int o = 0; o < 4; ++o) {
      if (o == turn) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float* rv = lv[wc * 64 + j * 32 + c];
          int* ri = li[wc * 64 + j * 32 + c];
          // The query's K-th best score, in a register: read INSIDE the turn (between two barriers this lane is the list's only writer
          // and nobody else reads it) and refreshed after every insertion, so a score that cannot enter costs one v_cmp and no LDS
          // access.  s >= thr lets through a superset of what the list accepts (equal scores: the index decides); knn_insert decides.
          // Queries past Nq take nothing.
          float thr = qok[j] ? rv[K - 1] : INFINITY;
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
              const int key = key0 + i * 32 + (e & 3) + 8 * (e >> 2);
              const float s = acc[i][j][e];
              if (s >= thr && key < nk && key != excl[j]) {
                knn_insert(rv, ri, K, s, key);
                thr = rv[K - 1];
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

// ------------------------------------------------------------------------------------------ 2. merge of the key splits
__global__ __launch_bounds__(KNN_FIN_THREADS) void knn_finish(const float* __restrict__ ws_val, const int32_t* __restrict__ ws_idx, int64_t Nq,
                                                              int splits, int K, int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
  __shared__ float lv[KNN_FIN_THREADS][KNN_LP];
  __shared__ int li[KNN_FIN_THREADS][KNN_LP];
  const int64_t i = (int64_t)blockIdx.x * KNN_FIN_THREADS + threadIdx.x;
  if (i >= Nq) return;                           // (no barrier below: a thread touches its own row only)
  float* rv = lv[threadIdx.x];
  int* ri = li[threadIdx.x];
  for (int p = 0; p < K; ++p) {
    rv[p] = -INFINITY;
    ri[p] = KNN_NONE;
  }
  for (int s = 0; s < splits; ++s) {             // ascending split = ascending key range: a fixed order
    const int64_t o = ((int64_t)s * Nq + i) * K;
    for (int p = 0; p < K; ++p) {
      const float v = ws_val[o + p];
      const int ix = ws_idx[o + p];
      if (ix == KNN_NONE || !knn_before(v, ix, rv[K - 1], ri[K - 1])) break;      // the split's list is ordered: nothing after this enters
      knn_insert(rv, ri, K, v, ix);
    }
  }
  for (int p = 0; p < K; ++p) {
    const int ix = ri[p];
    out_idx[i * K + p] = ix == KNN_NONE ? -1 : ix;
    out_val[i * K + p] = ix == KNN_NONE ? -INFINITY : rv[p];
  }
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_knn_ws_bytes(int64_t Nq, int64_t Nk, int64_t D, int K) {
  if (Nq <= 0 || Nk <= 0 || D <= 0 || K < 1 || K > KNN_KMAX || Nq > 0x7fffffff - RR_TQ || Nk > 0x7fffffff - RR_TK) return 0;   // what dinox_knn_topk refuses
  return knn_split(Nq, Nk).splits * Nq * K * 8;   // an ordered (score, index) list of K per query and key split
}

extern "C" int dinox_knn_topk(const float* q, int64_t ldq, const float* k, int64_t ldk, const int32_t* exclude, int64_t Nq, int64_t Nk, int64_t D,
                              int K, int32_t* out_idx, float* out_val, void* ws, void* stream) {
  DX_REQUIRE(K >= 1 && K <= KNN_KMAX, DINOX_EINVAL, "knn_topk: K=%d outside [1, %d]", K, KNN_KMAX);
  DX_REQUIRE(q && k && out_idx && out_val && ws, DINOX_EINVAL, "knn_topk: null pointer");
  DX_REQUIRE(Nq > 0 && Nk > 0 && D > 0 && Nq <= 0x7fffffff - RR_TQ && Nk <= 0x7fffffff - RR_TK && ldq >= D && ldk >= D, DINOX_EINVAL,   // (padded indices of the last tile stay in int)
             "knn_topk: Nq=%lld Nk=%lld D=%lld ldq=%lld ldk=%lld", (long long)Nq, (long long)Nk, (long long)D, (long long)ldq, (long long)ldk);
  const RrSplit sp = knn_split(Nq, Nk);
  const bool vec = (uintptr_t)q % 16 == 0 && (uintptr_t)k % 16 == 0 && ldq % 4 == 0 && ldk % 4 == 0 && D % 4 == 0;
  float* ws_val = (float*)ws;
  int32_t* ws_idx = (int32_t*)(ws_val + sp.splits * Nq * K);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)sp.strips, (unsigned)sp.splits);
#define KNN_SWEEP(V) \
  hipLaunchKernelGGL(knn_sweep<V>, grid, dim3(RR_THREADS), 0, st, q, ldq, k, ldk, exclude, Nq, Nk, D, K, sp.tiles_per_split, ws_val, ws_idx)
  if (vec) KNN_SWEEP(true); else KNN_SWEEP(false);
#undef KNN_SWEEP
  if (int rc = check_launch("knn_sweep")) return rc;
  hipLaunchKernelGGL(knn_finish, dim3((unsigned)ceil_div(Nq, (int64_t)KNN_FIN_THREADS)), dim3(KNN_FIN_THREADS), 0, st, (const float*)ws_val,
                     (const int32_t*)ws_idx, Nq, (int)sp.splits, K, out_idx, out_val);
  return check_launch("knn_finish");
}
