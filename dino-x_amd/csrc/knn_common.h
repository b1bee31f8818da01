// knn_common.h -- what the top-K sweeps share (knn.hip: the K nearest keys; labelprop.hip: the K nearest keys inside a spatial window, then
// a vote): the list geometry, the key-split policy, the total order and the insertion into an ordered list.  Both files select with the
// SAME order, so with a whole-grid window the lists are bitwise equal.
#pragma once
#include "retrieval_common.h"

namespace dinox {

constexpr int KNN_KMAX = 32;
constexpr int KNN_LP = KNN_KMAX + 1;             // list pitch: the 32 queries of a half-wave touch 32 different banks at equal depth
constexpr int KNN_NONE = 0x7fffffff;             // index of an empty slot (sorts after every key of equal score)
constexpr int KNN_FIN_THREADS = 64;

// Key splits: the rank kernel's policy, then longer splits while the grid stays large.  A split starts from an empty list and a query's
// threshold only tightens with the keys its split has seen, so the insertions per tile fall as 1 / (tiles seen): longer splits insert less
// (measured on MI355X, D = 384, K = 10, DESIGN.md "Neighbours": N = 16 384 with 8 / 16 / 32 tiles per split 5.44 / 5.00 / 4.13 ms) -- but not
// at the price of an empty chip (N = 4096 with 2 / 16 / 32 tiles per split, i.e. 512 / 64 / 32 workgroups: 0.78 / 2.21 / 3.33 ms).  So: double
// the tiles per split up to 32 while at least 512 workgroups remain.  A pure function of (Nq, Nk): workspace size and launch agree.
constexpr int64_t KNN_LONG_SPLIT = 32, KNN_MIN_GROUPS = 512;

static RrSplit knn_split(int64_t Nq, int64_t Nk) {
  RrSplit s = rr_split(Nq, Nk);
  const int64_t tiles = ceil_div(Nk, (int64_t)RR_TK);
  while (s.tiles_per_split < KNN_LONG_SPLIT && s.strips * ceil_div(tiles, 2 * s.tiles_per_split) >= KNN_MIN_GROUPS) s.tiles_per_split *= 2;
  s.splits = ceil_div(tiles, s.tiles_per_split);
  return s;
}

// the total order: score descending, index ascending
__device__ __forceinline__ bool knn_before(float v, int i, float w, int j) { return v > w || (v == w && i < j); }

// (s, key) into the ordered list of K entries if it comes before the last one; at most K - 1 moves
__device__ __forceinline__ void knn_insert(float* __restrict__ lv, int* __restrict__ li, int K, float s, int key) {
  if (!knn_before(s, key, lv[K - 1], li[K - 1])) return;
  int p = K - 1;
  while (p > 0) {
    const float w = lv[p - 1];
    const int j = li[p - 1];
    if (!knn_before(s, key, w, j)) break;
    lv[p] = w;
    li[p] = j;
    --p;
  }
  lv[p] = s;
  li[p] = key;
}

}  // namespace dinox
