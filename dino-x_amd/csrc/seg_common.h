// seg_common.h -- what segloss.hip, segcalib.hip, segrefine.hip and segblend.hip share: the register width that holds the C logits of a
// pixel, and (the first three) the walk over the pixels of a cell with its interpolation, the softmax of a pixel's logits and the size limits.
#pragma once
#include <type_traits>

#include "common.h"
#include "kernels.h"

namespace dinox {

static int seg_cp(int C) { return C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64; }

// f(std::integral_constant<int, CP>) for the register width that holds C classes
template <typename F>
static inline void seg_by_width(int C, F&& f) {
  switch (seg_cp(C)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// ---------------------------------------------------------------- the cell walk (layout: the head of segloss.hip)
constexpr int SEG_WAVES = 4;                      // waves (= cells in flight) per workgroup
constexpr int SEG_MAX_UPSAMPLE = 32;              // a cell (the pixels that share their four taps) is at most 1.5 u = 48 columns: one wave row

__device__ __forceinline__ int seg_lo(int k, int g, int u, int S) { return k <= 0 ? 0 : (k >= g ? S : k * u + u / 2); }

// weight of the second tap at pixel coordinate x of cell index k: frac((x + 0.5) / u - 0.5) as (2 x + 1 - u - 2 u k) / (2 u), 0 where the
// source coordinate is clamped at 0 or where the second tap is clamped onto the first (k = g - 1: both weights go to the one patch).
__device__ __forceinline__ float seg_w1(int x, int k, int g, int u, float inv2u) {
  const int t = 2 * x + 1 - u;
  return (k + 1 < g && t > 0) ? (float)(t - 2 * u * k) * inv2u : 0.f;
}

// Pixel column of `lane` in a cell of column index cx: the lanes run along the cell's rows, 64 / width rows at a time.
__device__ __forceinline__ int seg_lane_x(int cx, int g, int u, int lane) {
  const int xlo = seg_lo(cx, g, u, g * u), cw = seg_lo(cx + 1, g, u, g * u) - xlo;
  return xlo + lane % cw;
}

// Calls f(ok, lab, wy0, wy1, l, Y, X) for the pixels of `cell`, this lane's column from the top row down; l[c] = the interpolated logit.
// Every lane of the wave makes every call (ok = false where the lane has no pixel), so f may use wave-wide operations.
// y == nullptr: lab = 255 everywhere.  ywide: u % 8 == 0 and y 4-byte aligned -- every fourth lane reads four labels in one 32-bit load.
template <int CP, typename F>
__device__ __forceinline__ void seg_cell_pixels(const float* __restrict__ z, const uint8_t* __restrict__ y, int g, int u, int C, float inv2u, int ywide,
                                                int64_t cell, int lane, F&& f) {
  const int S = g * u;
  const int cx = (int)(cell % g), cy = (int)((cell / g) % g);
  const int64_t b = cell / ((int64_t)g * g);
  const int xlo = seg_lo(cx, g, u, S), xhi = seg_lo(cx + 1, g, u, S), ylo = seg_lo(cy, g, u, S), yhi = seg_lo(cy + 1, g, u, S);
  const int cw = xhi - xlo, R = 64 / cw;          // 1 <= cw <= 48
  const int r0 = lane / cw, X = seg_lane_x(cx, g, u, lane);
  const bool live = r0 < R;
  const float wx1 = seg_w1(X, cx, g, u, inv2u), wx0 = 1.f - wx1;
  const int cx1 = cx + 1 < g ? cx + 1 : cx, cy1 = cy + 1 < g ? cy + 1 : cy;
  const float* z00 = z + ((b * g + cy) * g + cx) * C;
  const float* z01 = z + ((b * g + cy) * g + cx1) * C;
  const float* z10 = z + ((b * g + cy1) * g + cx) * C;
  const float* z11 = z + ((b * g + cy1) * g + cx1) * C;
  float zx0[CP], zx1[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const bool in = c < C;
    zx0[c] = in ? wx0 * z00[c] + wx1 * z01[c] : 0.f;
    zx1[c] = in ? wx0 * z10[c] + wx1 * z11[c] : 0.f;
  }
  const uint8_t* yb = y ? y + b * (int64_t)S * S : nullptr;
  for (int Y0 = ylo; Y0 < yhi; Y0 += R) {          // wave-uniform trip count
    const int Y = Y0 + r0;
    const bool ok = live && Y < yhi;
    int lab = 255;
    if (yb) {
      if (ywide) {
        unsigned w = 0;
        if (ok && (lane & 3) == 0) w = *reinterpret_cast<const unsigned*>(yb + (int64_t)Y * S + X);
        w = __shfl(w, lane & ~3, 64);
        lab = ok ? (int)((w >> (8 * (lane & 3))) & 255u) : 255;
      } else if (ok) {
        lab = yb[(int64_t)Y * S + X];
      }
    }
    const float wy1 = seg_w1(Y, cy, g, u, inv2u), wy0 = 1.f - wy1;
    float l[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) l[c] = wy0 * zx0[c] + wy1 * zx1[c];
    f(ok, lab, wy0, wy1, l, Y, X);
  }
}

// l[c] of the one pixel (X, Y) of image b: the taps, the weights and the order of operations of seg_cell_pixels, for a kernel whose threads
// do not walk cells (csrc/segrefine.hip).  Pixel x lies in the cell of index max(x - u / 2, 0) / u (seg_lo).  The same expressions, not
// necessarily the same bits: the compiler fuses multiply-adds per kernel (and per class), so a value may differ in the last place.
template <int CP>
__device__ __forceinline__ void seg_pixel_logits(const float* __restrict__ z, int64_t b, int g, int u, int C, float inv2u, int X, int Y, float (&l)[CP]) {
  const int h = u / 2;
  const int cx = X > h ? (X - h) / u : 0, cy = Y > h ? (Y - h) / u : 0;
  const float wx1 = seg_w1(X, cx, g, u, inv2u), wx0 = 1.f - wx1;
  const float wy1 = seg_w1(Y, cy, g, u, inv2u), wy0 = 1.f - wy1;
  const int cx1 = cx + 1 < g ? cx + 1 : cx, cy1 = cy + 1 < g ? cy + 1 : cy;
  const float* z00 = z + ((b * g + cy) * g + cx) * C;
  const float* z01 = z + ((b * g + cy) * g + cx1) * C;
  const float* z10 = z + ((b * g + cy1) * g + cx) * C;
  const float* z11 = z + ((b * g + cy1) * g + cx1) * C;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const bool in = c < C;
    const float zx0 = in ? wx0 * z00[c] + wx1 * z01[c] : 0.f;
    const float zx1 = in ? wx0 * z10[c] + wx1 * z11[c] : 0.f;
    l[c] = wy0 * zx0 + wy1 * zx1;
  }
}

// s l as one rounded multiply: never contracted into a neighbouring addition, so every place that forms it gets the same bits.
__device__ __forceinline__ float seg_scaled(float s, float l) {
#pragma clang fp contract(off)
  return s * l;
}

// l -> p = softmax(l) in place over c < C; returns max and the sum of exp(l - max).
template <int CP>
__device__ __forceinline__ void seg_softmax(float (&l)[CP], int C, float& m, float& sum) {
  m = l[0];
#pragma unroll
  for (int c = 1; c < CP; ++c)
    if (c < C) m = fmaxf(m, l[c]);
  sum = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    l[c] = c < C ? expf(l[c] - m) : 0.f;
    sum += l[c];
  }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < CP; ++c) l[c] *= inv;
}

// ---------------------------------------------------------------- host: what the entry points over (B, g, u, C) check
static int seg_wide(const void* p, int u) { return u % 8 == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// The size limits, said once: 0 when (B, g, u, C) is inside all of them, else the number of the first one broken (seg_geometry words it).
// B g^2 cells and B S^2 pixels stay far inside int64 and the grids inside 2^31 - 1.
static int seg_broken_limit(int64_t B, int g, int u, int C) {
  if (!(B >= 1 && B <= (1 << 20) && g >= 1 && g <= 4096)) return 1;
  if (!(u >= 1 && u <= SEG_MAX_UPSAMPLE)) return 2;
  if (!(C >= 2)) return 3;
  if (!(C <= SEG_MAX_CLASSES)) return 4;
  if (!(B * g * g <= ((int64_t)1 << 32))) return 5;
  return 0;
}

// 0, or the error code after the message is set.
static int seg_geometry(const char* who, int64_t B, int g, int u, int C) {
  switch (seg_broken_limit(B, g, u, C)) {
    case 1: return fail(DINOX_EINVAL, "%s: B=%lld g=%d (1 <= B <= 2^20; 1 <= g <= 4096)", who, (long long)B, g);
    case 2: return fail(DINOX_EINVAL, "%s: u=%d (1 <= u <= %d)", who, u, SEG_MAX_UPSAMPLE);
    case 3: return fail(DINOX_EINVAL, "%s: C=%d (2 <= C <= %d)", who, C, SEG_MAX_CLASSES);
    case 4: return fail(DINOX_EUNSUPPORTED, "%s: C=%d classes: at most %d are held in registers", who, C, SEG_MAX_CLASSES);
    case 5: return fail(DINOX_EINVAL, "%s: B g^2 = %lld cells (at most 2^32)", who, (long long)(B * g * g));
  }
  return 0;
}

}  // namespace dinox
