// segrefine.hip -- edge-aware refinement of a dense segmenter's class probabilities: T mean-field iterations of a local CRF whose pairwise
// weights follow a guide image (definitions: include/dinox.h).  The unary term is the upsampled patch logits at an inverse temperature, so
// the arg-max can move to the grey-value edge that lies below the patch scale.
//
// Launches.  One over the cells (the walk, the interpolation and the softmax of seg_common.h) writes Q^0 into the first of two class-major
// planes Q[B][C][S][S]; one per iteration reads a plane and writes the other; the last iteration writes no plane: it takes the arg-max, the
// confidence and the counts in that same launch.  T = 0 is dinox_seg_predict and, for the confidence, dinox_seg_calib: their bits.
//
// The iteration kernel.  A workgroup owns a 32 x 8 pixel tile.  It stages the guide's tile plus a halo of r d pixels in LDS once, with
// the table of the halo's global offsets (-1 outside the image), and each thread forms the (2r+1)^2 - 1 weights g a of its pixel once, in
// registers (templated on r): an out-of-image neighbour has weight 0 and enters neither sum.  The class loop then stages Q_c's tile plus halo
// through the offset table (0 outside) and adds the window in the fixed order dy outer, dx inner, ascending; it never touches the guide or
// exp() again.  m[c] stays in the seg_by_width register array; the unary logits are re-interpolated per pixel (seg_pixel_logits) and the
// softmax is seg_softmax.  No address depends on a float; a non-finite logit or guide pixel spreads through the windows it lies in and
// nowhere else.  No floating-point atomic: equal inputs give equal bits.  Counts: integer atomics, LDS then global, as seg_predict_kernel.
#include "small_common.h"
#include "kernels.h"
#include "seg_common.h"

#include <cmath>

namespace dinox {

constexpr int SEG_REFINE_TW = 32, SEG_REFINE_TH = 8;          // the tile: one thread per pixel
constexpr int SEG_REFINE_THREADS = SEG_REFINE_TW * SEG_REFINE_TH;
constexpr int SEG_REFINE_MAX_ITERS = 32, SEG_REFINE_MAX_RADIUS = 3, SEG_REFINE_MAX_DILATION = 8;
constexpr int SEG_REFINE_MAX_TAPS = (2 * SEG_REFINE_MAX_RADIUS + 1) * (2 * SEG_REFINE_MAX_RADIUS + 1);

struct SegRefineTable {                                       // g_(dy,dx), row-major over the window; travels in the kernel arguments
  float g[SEG_REFINE_MAX_TAPS];
};

// pred, conf and the counters of one pixel; cnt[3 CP + 1] is seg_predict_kernel's LDS layout
template <int CP>
__device__ __forceinline__ void seg_refine_emit(uint8_t* __restrict__ pred, float* __restrict__ conf, unsigned* cnt, int64_t at, int best, float cf,
                                                int lab, int C) {
  pred[at] = (uint8_t)best;
  if (conf) conf[at] = cf;
  if (lab == 255) return;
  if (lab >= C) {
    atomicAdd(&cnt[3 * CP], 1u);
    return;
  }
  if (best == lab) atomicAdd(&cnt[best], 1u);
  atomicAdd(&cnt[CP + best], 1u);
  atomicAdd(&cnt[2 * CP + lab], 1u);
}

template <int CP>
__device__ __forceinline__ void seg_refine_flush(const unsigned* cnt, unsigned long long* __restrict__ counts, int C, int i, int stride) {
  for (; i < 3 * C + 1; i += stride) {
    const int t = i / C, c = i - t * C;
    const unsigned v = i == 3 * C ? cnt[3 * CP] : cnt[t * CP + c];
    if (v) atomicAdd(&counts[i], (unsigned long long)v);
  }
}

// Q^0 = softmax(s l) into the first plane: the cell walk, a wave per cell.
template <int CP>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_refine_init_kernel(const float* __restrict__ z, float s, float* __restrict__ Q, int g, int u, int C,
                                                                         float inv2u, int64_t ncell) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, S = g * u;
  const int64_t cell = (int64_t)blockIdx.x * SEG_WAVES + wave;
  if (cell >= ncell) return;
  const int64_t b = cell / ((int64_t)g * g), plane = (int64_t)S * S;
  seg_cell_pixels<CP>(z, nullptr, g, u, C, inv2u, 0, cell, lane, [&](bool ok, int, float, float, float(&l)[CP], int Y, int X) {
    float p[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) p[c] = seg_scaled(s, l[c]);
    float m, sum;
    seg_softmax<CP>(p, C, m, sum);
    if (!ok) return;
    const int64_t at = (int64_t)Y * S + X;
#pragma unroll
    for (int c = 0; c < CP; ++c)
      if (c < C) Q[(b * C + c) * plane + at] = p[c];
  });
}

// One iteration.  Qout != nullptr: Q^t into the plane.  Qout == nullptr (the last one): pred, conf, counts.
// Dynamic LDS: n = (TW + 2 H)(TH + 2 H) floats of the guide, n of Q_c, n ints of offsets; H = R d <= 24, so at most 53760 bytes.
template <int CP, int R>
__global__ __launch_bounds__(SEG_REFINE_THREADS) void seg_refine_iter_kernel(const float* __restrict__ z, const float* __restrict__ I,
                                                                             const uint8_t* __restrict__ y, const float* __restrict__ Qin,
                                                                             float* __restrict__ Qout, uint8_t* __restrict__ pred,
                                                                             float* __restrict__ conf, unsigned long long* __restrict__ counts,
                                                                             SegRefineTable tab, int g, int u, int C, int d, float inv2u,
                                                                             float inv2sI2, float lambda, float w, float s, int tiles_x, int tiles_y) {
  constexpr int K = 2 * R + 1;
  extern __shared__ float seg_refine_lds[];
  __shared__ unsigned cnt[3 * CP + 1];
  const int S = g * u, H = R * d, LW = SEG_REFINE_TW + 2 * H, LH = SEG_REFINE_TH + 2 * H, n = LW * LH;
  float* gI = seg_refine_lds;
  float* q = seg_refine_lds + n;
  int* goff = reinterpret_cast<int*>(seg_refine_lds + 2 * n);
  const int tid = threadIdx.x, tx = tid % SEG_REFINE_TW, ty = tid / SEG_REFINE_TW;
  const int64_t blk = blockIdx.x;
  const int x0 = (int)(blk % tiles_x) * SEG_REFINE_TW, y0 = (int)((blk / tiles_x) % tiles_y) * SEG_REFINE_TH;
  const int64_t b = blk / ((int64_t)tiles_x * tiles_y), plane = (int64_t)S * S;
  const int X = x0 + tx, Y = y0 + ty;
  const bool live = X < S && Y < S;
  const int64_t org = (int64_t)(y0 - H) * S + (x0 - H);       // the halo's first pixel (outside the image where negative: never read)
  for (int i = tid; i < n; i += SEG_REFINE_THREADS) {
    const int ry = i / LW, rx = i - ry * LW, gy = y0 - H + ry, gx = x0 - H + rx;
    const bool in = gy >= 0 && gy < S && gx >= 0 && gx < S;
    const int off = in ? ry * S + rx : -1;                    // <= 56 * 2^17
    goff[i] = off;
    gI[i] = in ? I[b * plane + org + off] : 0.f;
  }
  for (int i = tid; i < 3 * CP + 1; i += SEG_REFINE_THREADS) cnt[i] = 0;
  __syncthreads();

  // the weights of this pixel's window and their normaliser, once
  const int ctr = (ty + H) * LW + tx + H;
  const float Ip = gI[ctr], oml = 1.f - lambda;
  float wgt[K * K], norm = 0.f;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const int k = (dy + R) * K + dx + R;
      if (dy == 0 && dx == 0) {
        wgt[k] = 0.f;
        continue;
      }
      const int jy = Y + dy * d, jx = X + dx * d;
      const bool in = jy >= 0 && jy < S && jx >= 0 && jx < S;
      const float dI = Ip - gI[ctr + dy * d * LW + dx * d];
      const float a = oml + lambda * expf(-(dI * dI) * inv2sI2);
      wgt[k] = in ? tab.g[k] * a : 0.f;
      norm += in ? tab.g[k] : 0.f;
    }

  float acc[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    acc[c] = 0.f;
    if (c < C) {                                              // uniform
      __syncthreads();                                        // the reads of the class before are done
      const int64_t base = (b * C + c) * plane + org;
      for (int i = tid; i < n; i += SEG_REFINE_THREADS) {
        const int off = goff[i];
        q[i] = off >= 0 ? Qin[base + off] : 0.f;
      }
      __syncthreads();
      float a = 0.f;
#pragma unroll
      for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx)
          if (dy != 0 || dx != 0) a += wgt[(dy + R) * K + dx + R] * q[ctr + dy * d * LW + dx * d];
      acc[c] = a;
    }
  }

  if (live) {
    float v[CP];
    seg_pixel_logits<CP>(z, b, g, u, C, inv2u, X, Y, v);
#pragma unroll
    for (int c = 0; c < CP; ++c) v[c] = c < C ? seg_scaled(s, v[c]) + w * (acc[c] / norm) : 0.f;
    int best = 0;
    float bv = v[0];
#pragma unroll
    for (int c = 1; c < CP; ++c)
      if (c < C && v[c] > bv) bv = v[c], best = c;
    float m, sum;
    seg_softmax<CP>(v, C, m, sum);
    const int64_t at = (int64_t)Y * S + X;
    if (Qout) {                                               // uniform
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C) Qout[(b * C + c) * plane + at] = v[c];
    } else {
      float cf = v[0];
#pragma unroll
      for (int c = 1; c < CP; ++c) cf = best == c ? v[c] : cf;
      seg_refine_emit<CP>(pred + b * plane, conf ? conf + b * plane : nullptr, cnt, at, best, cf, y ? (int)y[b * plane + at] : 255, C);
    }
  }
  if (!Qout && counts) {                                      // uniform
    __syncthreads();
    seg_refine_flush<CP>(cnt, counts, C, tid, SEG_REFINE_THREADS);
  }
}

// tiles of the whole batch, or 0 where S^2 planes or the grid leave their ranges
static int64_t seg_refine_tiles(int64_t B, int g, int u) {
  const int64_t S = (int64_t)g * u;
  const int64_t tiles = B * ceil_div(S, (int64_t)SEG_REFINE_TW) * ceil_div(S, (int64_t)SEG_REFINE_TH);
  return tiles <= 0x7fffffff ? tiles : 0;
}

template <int CP, int R, typename... A>
static void seg_refine_launch_iter(unsigned grid, size_t lds, hipStream_t st, A... a) {
  hipLaunchKernelGGL((seg_refine_iter_kernel<CP, R>), dim3(grid), dim3(SEG_REFINE_THREADS), lds, st, a...);
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
extern "C" int64_t dinox_seg_refine_ws_bytes(int64_t B, int g, int u, int C) {
  if (seg_broken_limit(B, g, u, C) || !seg_refine_tiles(B, g, u)) return 0;
  const int64_t S = (int64_t)g * u;
  if (B * C * S * S > ((int64_t)1 << 40)) return 0;
  return 2 * B * C * S * S * (int64_t)sizeof(float);
}

extern "C" int dinox_seg_refine(const float* z, const float* I, const uint8_t* y, uint8_t* pred, float* conf, int64_t* counts, void* ws, int64_t B,
                                int g, int u, int C, int T, int r, int d, const float* gtab, float inv2sI2, float lambda, float w, float s,
                                void* stream) {
  int rc = seg_geometry("seg_refine", B, g, u, C);
  if (rc) return rc;
  const int64_t S = (int64_t)g * u;
  DX_REQUIRE(dinox_seg_refine_ws_bytes(B, g, u, C) > 0, DINOX_EINVAL, "seg_refine: B=%lld S=%lld C=%d: more than 2^31 - 1 tiles or 2^40 plane elements",
             (long long)B, (long long)S, C);
  DX_REQUIRE(T >= 0 && T <= SEG_REFINE_MAX_ITERS, DINOX_EINVAL, "seg_refine: T=%d iterations (0 <= T <= %d)", T, SEG_REFINE_MAX_ITERS);
  DX_REQUIRE(r >= 1 && r <= SEG_REFINE_MAX_RADIUS, DINOX_EINVAL, "seg_refine: r=%d (1 <= r <= %d)", r, SEG_REFINE_MAX_RADIUS);
  DX_REQUIRE(d >= 1 && d <= SEG_REFINE_MAX_DILATION, DINOX_EINVAL, "seg_refine: d=%d (1 <= d <= %d)", d, SEG_REFINE_MAX_DILATION);
  DX_REQUIRE((int64_t)r * d < S, DINOX_EINVAL, "seg_refine: r d = %d reaches across the image side S = %lld (r d < S)", r * d, (long long)S);
  // a pixel with S - d <= x < d and S - d <= y < d would have every offset outside the image: an empty N(p), a normaliser of 0
  DX_REQUIRE(2 * (int64_t)d <= S, DINOX_EINVAL, "seg_refine: d = %d leaves the pixels in the middle of an image of side S = %lld no neighbour (2 d <= S)", d,
             (long long)S);
  DX_REQUIRE(s > 0.f && std::isfinite(s), DINOX_EINVAL, "seg_refine: inv_temperature=%g (finite and > 0)", (double)s);
  DX_REQUIRE(inv2sI2 >= 0.f && std::isfinite(inv2sI2), DINOX_EINVAL, "seg_refine: 1 / (2 sigma_I^2) = %g (finite and >= 0)", (double)inv2sI2);
  DX_REQUIRE(lambda >= 0.f && lambda <= 1.f, DINOX_EINVAL, "seg_refine: lambda=%g (0 <= lambda <= 1)", (double)lambda);
  DX_REQUIRE(w >= 0.f && std::isfinite(w), DINOX_EINVAL, "seg_refine: w=%g (finite and >= 0)", (double)w);
  DX_REQUIRE(z && I && pred && gtab, DINOX_EINVAL, "seg_refine: null pointer (z, I, pred or gtab)");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "seg_refine: labels and counts come together (both or neither)");
  DX_REQUIRE(T == 0 || ws, DINOX_EINVAL, "seg_refine: T=%d needs the workspace of dinox_seg_refine_ws_bytes (ws is null)", T);
  const int K = 2 * r + 1;
  SegRefineTable tab = {};
  for (int k = 0; k < K * K; ++k) {
    const int dy = k / K - r, dx = k % K - r;
    const bool nearest = (dy == 0 && (dx == 1 || dx == -1)) || (dx == 0 && (dy == 1 || dy == -1));
    DX_REQUIRE(std::isfinite(gtab[k]) && gtab[k] >= 0.f && (!nearest || gtab[k] > 0.f), DINOX_EINVAL,
               "seg_refine: gtab[%d] = %g (finite and >= 0; > 0 at the four nearest neighbours, so that no normaliser is 0)", k, (double)gtab[k]);
    tab.g[k] = gtab[k];
  }
  hipStream_t st = as_stream(stream);
  if (counts && T > 0) {                          // (at T = 0 dinox_seg_predict zeroes them)
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)(3 * C + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) return fail((int)e, "seg_refine: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  const int64_t ncell = B * g * g, plane_all = B * C * S * S;
  const float inv2u = 1.0f / (float)(2 * u);
  if (T == 0) {                                   // the two kernels themselves: their bits by construction
    rc = dinox_seg_predict(z, y, pred, counts, B, g, u, C, stream);
    if (rc || !conf) return rc;
    return dinox_seg_calib(z, nullptr, s, nullptr, conf, nullptr, nullptr, nullptr, nullptr, B, g, u, C, 1, stream);
  }
  float* Q0 = (float*)ws;
  float* Q1 = Q0 + plane_all;
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_refine_init_kernel<decltype(cp)::value>), dim3((unsigned)ceil_div(ncell, (int64_t)SEG_WAVES)), dim3(64 * SEG_WAVES), 0, st, z, s,
                       Q0, g, u, C, inv2u, ncell);
  });
  rc = check_launch("seg_refine (Q0)");
  if (rc) return rc;
  const int H = r * d, tiles_x = (int)ceil_div(S, (int64_t)SEG_REFINE_TW), tiles_y = (int)ceil_div(S, (int64_t)SEG_REFINE_TH);
  const unsigned grid = (unsigned)seg_refine_tiles(B, g, u);
  const size_t lds = (size_t)3 * (SEG_REFINE_TW + 2 * H) * (SEG_REFINE_TH + 2 * H) * sizeof(float);
  for (int t = 1; t <= T; ++t) {
    const float* Qin = (t & 1) ? Q0 : Q1;
    float* Qout = t == T ? nullptr : ((t & 1) ? Q1 : Q0);
    seg_by_width(C, [&](auto cp) {
      constexpr int CP = decltype(cp)::value;
      auto go = [&](auto rr) {
        seg_refine_launch_iter<CP, decltype(rr)::value>(grid, lds, st, z, I, y, Qin, Qout, pred, conf, (unsigned long long*)counts, tab, g, u, C, d,
                                                        inv2u, inv2sI2, lambda, w, s, tiles_x, tiles_y);
      };
      if (r == 1) go(std::integral_constant<int, 1>{});
      else if (r == 2) go(std::integral_constant<int, 2>{});
      else go(std::integral_constant<int, 3>{});
    });
    rc = check_launch("seg_refine (iteration)");
    if (rc) return rc;
  }
  return 0;
}
