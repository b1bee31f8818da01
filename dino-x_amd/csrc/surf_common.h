// surf_common.h -- what the two surface-distance files share: surfdist.hip (a batch of [H][W] maps) and surfdist3d.hip (one [Z][H][W]
// volume) read the same label maps, mark the same sets, keep the same sentinels in their distance planes and pick the k-th smallest
// distance by the same 8-bit radix select on fp32 bit patterns (definitions: include/dinox.h).
#pragma once
#include "small_common.h"
#include "kernels.h"

namespace dinox {

constexpr int SURF_MAX_SIDE = 1024;                // a line of squared distances (4 KiB) sits in LDS; an axis distance fits uint16 beside its sentinel
constexpr int SURF_MAX_TOL = 8;                    // tolerance counters per lane, in registers
constexpr unsigned SURF_NONE = 0xffffu;            // axis distance: no border element on this axis line (a real one is at most 1023)
constexpr float SURF_SKIP = -1.0f;                 // distance plane: not a border element of the query side (sign bit set)
constexpr unsigned SURF_INF = 0x7f800000u;         // distance plane: the other side has no border at all

struct SurfTol {
  float v[SURF_MAX_TOL];
};

// The element at index i is in the set of (plane, c): pred: gt != 255 and pred == c; gt: gt == c.  A label is compared, never an address.
__device__ __forceinline__ bool surf_member(const uint8_t* __restrict__ pb, const uint8_t* __restrict__ gb, int64_t i, int plane, int c) {
  const int g = gb[i];
  return plane == 0 ? (g != 255 && pb[i] == c) : g == c;
}

// The value v of plane (0: pred, 1: gt) belongs to no class: pred >= C, gt >= C other than 255.
__device__ __forceinline__ bool surf_bad_label(int v, int plane, int C) { return v >= C && (plane == 0 || v != 255); }

// ---------------------------------------------------------------- the radix select on the bit patterns of non-negative fp32 values
// Four rounds, shift = 24, 16, 8, 0.  A value takes part in a round if its digits above the round's agree with the prefix chosen so far.
__device__ __forceinline__ bool surf_radix_takes_part(unsigned bits, unsigned prefix, int shift) {
  return shift == 24 || (bits >> (shift + 8)) == (prefix >> (shift + 8));
}
// The digit whose bin holds the k-th smallest (1 <= k <= the histogram's population); k becomes the rank inside that bin.
__device__ __forceinline__ unsigned surf_radix_pick(const unsigned* hist, unsigned& k) {
  unsigned digit = 0;
  while (digit < 255 && hist[digit] < k) k -= hist[digit++];
  return digit;
}

}  // namespace dinox
