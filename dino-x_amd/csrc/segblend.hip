// segblend.hip -- sliding-window prediction at native resolution: the window-weighted blend of overlapping tiles' patch logits, their
// bilinear upsampling (align_corners = False, any tile side, not only a multiple of the patch grid), the arg-max, the confidence and the
// confusion counts in one gather launch (definitions: include/dinox.h).
//
// Layout.  A WAVE takes a run of 64 consecutive pixels of one image row, so everything that depends on the row alone is wave-uniform:
// the range of tile rows that cover it, their window weights, their two patch rows and the weight between them (ys, flips and the y side
// of win are read at uniform addresses).  The tile columns that touch the run are a uniform range too; inside it a lane tests whether the
// tile covers its own pixel.  Per covering tile a lane reads four logit rows of C floats, interpolates them and adds w l_c to C
// accumulators in registers, in the order variant, tile row, tile column -- the order is the pixel's own, so no sum ever crosses lanes,
// nothing is scattered and no floating-point atomic exists.  The counts are integers: LDS atomics per wave, then one global 64-bit
// atomic per non-zero counter, as in seg_predict_kernel.
// Addresses: a tile index comes from a loop bound (< ny, < nx), a tile-local coordinate is used only after 0 <= l < t was tested, and a
// patch index is clamped into [0, g): no content of ys, xs, flips or z can move a load outside z or win, or a store outside the pixel's own.
#include "small_common.h"
#include "kernels.h"
#include "seg_common.h"

namespace dinox {

constexpr int SB_WAVES = 4;                       // waves (= 64-pixel runs) per workgroup

// One axis of the upsampling at tile-local coordinate l (0 <= l < t), mirrored first if `mirror`: the first tap k0, the second k1 and the
// weight of the second.  s = ((2 l + 1) g - t) / (2 t); negative: clamped to 0 (both taps 0 and 1, weight 0).
struct SbTap {
  int k0, k1, lm;
  float w1;
};
__device__ __forceinline__ SbTap sb_tap(int l, bool mirror, int g, int t, float inv2t) {
  SbTap r;
  r.lm = mirror ? t - 1 - l : l;
  const int n = (2 * r.lm + 1) * g - t;           // (host: t g <= 2^28)
  r.k0 = n > 0 ? (int)((unsigned)n / (unsigned)(2 * t)) : 0;
  r.k1 = r.k0 + 1 < g ? r.k0 + 1 : g - 1;
  r.w1 = (r.k0 + 1 < g && n > 0) ? (float)(n - 2 * t * r.k0) * inv2t : 0.f;
  return r;
}

template <int CP>
__global__ __launch_bounds__(64 * SB_WAVES) void seg_blend_predict_kernel(const float* __restrict__ z, const int* __restrict__ ys, const int* __restrict__ xs,
                                                                          const int* __restrict__ flips, const float* __restrict__ win,
                                                                          const uint8_t* __restrict__ y, uint8_t* __restrict__ pred,
                                                                          float* __restrict__ conf, unsigned long long* __restrict__ counts, int F, int ny,
                                                                          int nx, int g, int t, int C, int H, int W, float inv2t, int nxr, int64_t nrun,
                                                                          int pwide) {
  __shared__ unsigned cnt[SB_WAVES][3 * CP + 1];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (int i = lane; i < 3 * CP + 1; i += 64) cnt[wave][i] = 0;
  __syncthreads();
  const int64_t run = (int64_t)blockIdx.x * SB_WAVES + wave;
  const bool live = run < nrun;                   // uniform
  if (live) {
    const int xr = (int)(run % nxr), Y = (int)((run / nxr) % H);
    const int64_t b = run / ((int64_t)nxr * H);
    const int x_first = xr * 64, x_last = x_first + 63 < W ? x_first + 63 : W - 1, X = x_first + lane;
    const bool ok = X < W;
    // the covering ranges: tile rows with ys <= Y < ys + t, tile columns that reach into [x_first, x_last] (ascending tables)
    int iy_lo = 0, iy_hi = 0, ix_lo = 0, ix_hi = 0;
    for (int i = 0; i < ny; ++i) {
      const int o = ys[i];
      iy_lo = o + t <= Y ? i + 1 : iy_lo;
      iy_hi = o <= Y ? i + 1 : iy_hi;
    }
    for (int i = 0; i < nx; ++i) {
      const int o = xs[i];
      ix_lo = o + t <= x_first ? i + 1 : ix_lo;
      ix_hi = o <= x_last ? i + 1 : ix_hi;
    }
    float acc[CP], wsum = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) acc[c] = 0.f;
    const int64_t tile_sz = (int64_t)g * g * C;
    for (int f = 0; f < F; ++f) {
      const int fl = flips[f];
      for (int iy = iy_lo; iy < iy_hi; ++iy) {
        const int ly = Y - ys[iy];
        if ((unsigned)ly >= (unsigned)t) continue;                // uniform; a table that is not ascending costs pixels, never an address
        const SbTap ty = sb_tap(ly, (fl & 2) != 0, g, t, inv2t);
        const float wyw = win[ty.lm], wy1 = ty.w1, wy0 = 1.f - wy1;
        const float* zrow = z + (((b * F + f) * ny + iy) * (int64_t)nx) * tile_sz;
        for (int ix = ix_lo; ix < ix_hi; ++ix) {
          const int lx = X - xs[ix];
          if (!ok || (unsigned)lx >= (unsigned)t) continue;       // per lane: no wave-wide operation below
          const SbTap tx = sb_tap(lx, (fl & 1) != 0, g, t, inv2t);
          const float w = wyw * win[tx.lm], wx1 = tx.w1, wx0 = 1.f - wx1;
          const float* zt = zrow + ix * tile_sz;
          const float* z00 = zt + ((int64_t)ty.k0 * g + tx.k0) * C;
          const float* z01 = zt + ((int64_t)ty.k0 * g + tx.k1) * C;
          const float* z10 = zt + ((int64_t)ty.k1 * g + tx.k0) * C;
          const float* z11 = zt + ((int64_t)ty.k1 * g + tx.k1) * C;
          if (C == CP) {                                          // uniform: whole rows, loads the compiler may widen
#pragma unroll
            for (int c = 0; c < CP; ++c) {
              const float a0 = wx0 * z00[c] + wx1 * z01[c], a1 = wx0 * z10[c] + wx1 * z11[c];
              acc[c] += w * (wy0 * a0 + wy1 * a1);
            }
          } else {
#pragma unroll
            for (int c = 0; c < CP; ++c) {
              if (c < C) {
                const float a0 = wx0 * z00[c] + wx1 * z01[c], a1 = wx0 * z10[c] + wx1 * z11[c];
                acc[c] += w * (wy0 * a0 + wy1 * a1);
              }
            }
          }
          wsum += w;
        }
      }
    }
    // the blended logits, their arg-max (lowest index on a tie; a NaN never wins, so best stays inside [0, C)) and the confidence
    int best = 0;
    float bv = acc[0] = acc[0] / wsum;
#pragma unroll
    for (int c = 1; c < CP; ++c) {
      if (c < C) {
        acc[c] = acc[c] / wsum;
        if (acc[c] > bv) bv = acc[c], best = c;
      }
    }
    const int64_t pix = (b * H + Y) * (int64_t)W + X;
    if (pwide) {                                  // W % 4 == 0 and pred 4-byte aligned: four lanes' bytes leave as one 32-bit store
      unsigned v = (unsigned)best << (8 * (lane & 3));
      v |= __shfl_xor(v, 1, 64);
      v |= __shfl_xor(v, 2, 64);
      if (ok && (lane & 3) == 0) *reinterpret_cast<unsigned*>(pred + pix) = v;
    } else if (ok) {
      pred[pix] = (uint8_t)best;
    }
    if (ok) {
      if (conf) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) s += c < C ? expf(acc[c] - bv) : 0.f;
        conf[pix] = 1.f / s;
      }
      if (y) {
        const int lab = y[pix];
        if (lab != 255) {
          if (lab >= C) {
            atomicAdd(&cnt[wave][3 * CP], 1u);
          } else {
            if (best == lab) atomicAdd(&cnt[wave][best], 1u);
            atomicAdd(&cnt[wave][CP + best], 1u);
            atomicAdd(&cnt[wave][2 * CP + lab], 1u);
          }
        }
      }
    }
  }
  __syncthreads();
  if (live && counts) {
    if (lane < C)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (cnt[wave][k * CP + lane]) atomicAdd(&counts[k * C + lane], (unsigned long long)cnt[wave][k * CP + lane]);
    if (lane == 0 && cnt[wave][3 * CP]) atomicAdd(&counts[3 * C], (unsigned long long)cnt[wave][3 * CP]);
  }
}

}  // namespace dinox

using namespace dinox;

extern "C" int dinox_seg_blend_predict(const float* z, const int32_t* ys, const int32_t* xs, const int32_t* flips, const float* win, const uint8_t* y,
                                       uint8_t* pred, float* conf, int64_t* counts, int64_t B, int F, int ny, int nx, int g, int t, int C, int H, int W,
                                       void* stream) {
  DX_REQUIRE(z && ys && xs && flips && win && pred, DINOX_EINVAL, "seg_blend_predict: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "seg_blend_predict: labels and counts come together (both or neither)");
  DX_REQUIRE(F >= 1 && F <= 4, DINOX_EINVAL, "seg_blend_predict: F=%d flip variants (1 <= F <= 4)", F);
  DX_REQUIRE(B >= 1 && B <= (1 << 20) && ny >= 1 && nx >= 1 && ny <= (1 << 20) && nx <= (1 << 20), DINOX_EINVAL,
             "seg_blend_predict: B=%lld ny=%d nx=%d (T = B F ny nx >= 1; B, ny, nx <= 2^20)", (long long)B, ny, nx);
  DX_REQUIRE(g >= 1 && g <= 4096, DINOX_EINVAL, "seg_blend_predict: g=%d (1 <= g <= 4096)", g);
  DX_REQUIRE(H >= 1 && W >= 1 && H <= (1 << 20) && W <= (1 << 20), DINOX_EINVAL, "seg_blend_predict: H=%d W=%d (1 <= H, W <= 2^20)", H, W);
  DX_REQUIRE(t >= 1 && t <= (H < W ? H : W), DINOX_EINVAL, "seg_blend_predict: t=%d (1 <= t <= min(H, W) = %d)", t, H < W ? H : W);
  DX_REQUIRE((int64_t)t * g <= ((int64_t)1 << 28), DINOX_EINVAL, "seg_blend_predict: t g = %lld (at most 2^28)", (long long)t * g);
  DX_REQUIRE(C >= 2, DINOX_EINVAL, "seg_blend_predict: C=%d (2 <= C <= %d)", C, SEG_MAX_CLASSES);
  DX_REQUIRE(C <= SEG_MAX_CLASSES, DINOX_EUNSUPPORTED, "seg_blend_predict: C=%d classes: at most %d are held in registers", C, SEG_MAX_CLASSES);
  const int nxr = (int)ceil_div(W, 64);
  const int64_t nrun = B * H * nxr;
  DX_REQUIRE(nrun <= ((int64_t)1 << 32), DINOX_EINVAL, "seg_blend_predict: B H ceil(W / 64) = %lld runs (at most 2^32)", (long long)nrun);
  hipStream_t st = as_stream(stream);
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)(3 * C + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) return fail((int)e, "seg_blend_predict: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  const unsigned grid = (unsigned)ceil_div(nrun, (int64_t)SB_WAVES);
  const float inv2t = 1.0f / (float)(2 * t);
  const int pwide = W % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 3) == 0;
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_blend_predict_kernel<decltype(cp)::value>), dim3(grid), dim3(64 * SB_WAVES), 0, st, z, ys, xs, flips, win, y, pred, conf,
                       (unsigned long long*)counts, F, ny, nx, g, t, C, H, W, inv2t, nxr, nrun, pwide);
  });
  return check_launch("seg_blend_predict");
}
