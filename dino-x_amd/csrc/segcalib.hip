// segcalib.hip -- how far the probabilities of a dense segmenter can be trusted, from the patch logits: per pixel the arg-max, its softmax
// probability at an inverse temperature s (the confidence) and the normalised entropy; against labels the reliability histogram and the
// sums behind NLL, Brier score and the Newton step of temperature fitting (definitions: include/dinox.h).  No full-resolution logit or
// probability tensor exists: the cell walk, the interpolation and the softmax are segloss.hip's (seg_common.h), a wave takes a cell, a
// lane a pixel column, and the C logits of a pixel, their softmax and every per-class term live in registers.
//
// The arg-max is taken on the interpolated logits BEFORE they are scaled, by the comparison loop of seg_predict_kernel, so pred is that
// kernel's map whatever s is (s > 0 keeps the order of distinct values but can round two of them onto one).
// Histogram: integers only -- per bin the pixel count, the correct ones and the confidences in 2^-24 fixed point -- added by integer
// atomics (64-bit, LDS per wave, then global), so it is exact and independent of the order.  The bin index is clamped by comparisons
// before it addresses LDS and a pixel whose confidence is not finite enters no bin: no address depends on unchecked float bits.
// Sums: the fixed order of seg_fwd_partial_kernel / seg_fwd_final_kernel -- a lane adds its pixels in row order, the wave butterfly,
// partial sums in the workspace by plain stores, a second launch adds them ascending.  No floating-point atomic.
#include "small_common.h"
#include "kernels.h"
#include "seg_common.h"

#include <cmath>

namespace dinox {

constexpr int SEG_CALIB_CELLS = 4;                // cells per partial sum (and per flush of a wave's LDS histogram) when there are labels
constexpr int SEG_CALIB_MAX_BINS = 64;
constexpr int SEG_CALIB_SUMS = 5;                 // NLL, Brier, G, H, entropy
constexpr int SEG_CALIB_SLOTS = 3 * SEG_CALIB_MAX_BINS + 3;

// seg_scaled (s l as one rounded multiply): seg_common.h -- csrc/segrefine.hip forms the same bits

// cnt[wave][3 k + (0, 1, 2)] = bin k's (count, correct, Q); cnt[wave][3 * 64 + (0, 1, 2)] = (valid pixels, labels >= C other than 255, valid
// pixels whose confidence is not finite).  wsf[part][5]: the five sums of the part's cells.  y == nullptr: hist and wsf are nullptr too and
// only the maps are written.  pred, conf, ent: each may be nullptr.
template <int CP>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_calib_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, float s, float inv_logc,
                                                                   uint8_t* __restrict__ pred, float* __restrict__ conf, float* __restrict__ ent,
                                                                   unsigned long long* __restrict__ hist, float* __restrict__ wsf, int g, int u, int C,
                                                                   int NB, float inv2u, int ywide, int pwide, int64_t ncell, int cells_per_part,
                                                                   int64_t nparts) {
  __shared__ unsigned long long cnt[SEG_WAVES][SEG_CALIB_SLOTS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, S = g * u;
  const int64_t part = (int64_t)blockIdx.x * SEG_WAVES + wave;
  for (int i = lane; i < SEG_CALIB_SLOTS; i += 64) cnt[wave][i] = 0ull;
  __syncthreads();
  float acc[SEG_CALIB_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (part < nparts) {
    const int64_t c_end = (part + 1) * cells_per_part < ncell ? (part + 1) * cells_per_part : ncell;
    for (int64_t cell = part * cells_per_part; cell < c_end; ++cell) {
      const int64_t img = (cell / ((int64_t)g * g)) * (int64_t)S * S;
      seg_cell_pixels<CP>(z, y, g, u, C, inv2u, ywide, cell, lane, [&](bool ok, int lab, float, float, float(&l)[CP], int Y, int X) {
        int best = 0;                             // seg_predict_kernel's loop, on the unscaled logits
        float bv = l[0];
#pragma unroll
        for (int c = 1; c < CP; ++c)
          if (c < C && l[c] > bv) bv = l[c], best = c;
        const int64_t at = img + (int64_t)Y * S + X;
        if (pred) {                               // uniform
          if (pwide) {                            // four lanes' bytes leave as one 32-bit store
            unsigned w = (unsigned)best << (8 * (lane & 3));
            w |= __shfl_xor(w, 1, 64);
            w |= __shfl_xor(w, 2, 64);
            if (ok && (lane & 3) == 0) *reinterpret_cast<unsigned*>(pred + at) = w;
          } else if (ok) {
            pred[at] = (uint8_t)best;
          }
        }
        float p[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) p[c] = seg_scaled(s, l[c]);
        float m, sum;
        seg_softmax<CP>(p, C, m, sum);
        float cf = p[0];
#pragma unroll
        for (int c = 1; c < CP; ++c) cf = best == c ? p[c] : cf;
        const float lse = logf(sum) + m;
        // a class of probability 0 contributes 0 to every p-weighted sum (also where its logit is -inf)
        float pt = 0.f, mu = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const bool on = p[c] > 0.f;
          pt += on ? p[c] * seg_scaled(s, l[c]) : 0.f;
          mu += on ? p[c] * l[c] : 0.f;
        }
        float e = (lse - pt) * inv_logc;
        e = e < 0.f ? 0.f : (e > 1.f ? 1.f : e);  // a NaN fails both comparisons and stays
        if (ok) {
          if (conf) conf[at] = cf;
          if (ent) ent[at] = e;
        }
        if (!ok || lab == 255) return;            // no wave-wide operation below
        if (lab >= C) {
          atomicAdd(&cnt[wave][3 * SEG_CALIB_MAX_BINS + 1], 1ull);
          return;
        }
        atomicAdd(&cnt[wave][3 * SEG_CALIB_MAX_BINS], 1ull);
        if (!(fabsf(cf) <= 3.402823466e38f)) {    // NaN or infinite: counted, in no bin and in no sum
          atomicAdd(&cnt[wave][3 * SEG_CALIB_MAX_BINS + 2], 1ull);
          return;
        }
        const float fb = cf * (float)NB;          // the float is compared first: only a value inside [0, NB) is converted
        const int k = fb >= (float)NB ? NB - 1 : (fb > 0.f ? (int)fb : 0);
        float fq = rintf(cf * 16777216.f);
        fq = fq > 33554432.f ? 33554432.f : (fq > 0.f ? fq : 0.f);
        atomicAdd(&cnt[wave][3 * k], 1ull);
        if (best == lab) atomicAdd(&cnt[wave][3 * k + 1], 1ull);
        atomicAdd(&cnt[wave][3 * k + 2], (unsigned long long)fq);
        float ly = 0.f, brier = 0.f, var = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          const bool hit = lab == c;
          ly = hit ? l[c] : ly;
          const float d = p[c] - (hit ? 1.f : 0.f), dl = l[c] - mu;
          brier += d * d;
          var += p[c] > 0.f ? p[c] * (dl * dl) : 0.f;
        }
        acc[0] += lse - seg_scaled(s, ly);
        acc[1] += brier;
        acc[2] += mu - ly;
        acc[3] += var;
        acc[4] += e;
      });
    }
  }
  if (wsf) {                                      // uniform
#pragma unroll
    for (int j = 0; j < SEG_CALIB_SUMS; ++j) {
      const float a = wave_sum(acc[j]);
      if (part < nparts && lane == 0) wsf[part * SEG_CALIB_SUMS + j] = a;
    }
  }
  __syncthreads();                                // the LDS counters of every wave are complete
  if (hist && part < nparts) {
    for (int i = lane; i < 3 * NB; i += 64)
      if (cnt[wave][i]) atomicAdd(&hist[i], cnt[wave][i]);
    if (lane < 3 && cnt[wave][3 * SEG_CALIB_MAX_BINS + lane]) atomicAdd(&hist[3 * NB + lane], cnt[wave][3 * SEG_CALIB_MAX_BINS + lane]);
  }
}

// One workgroup: sums[q] = the parts' q-th sums in a fixed order (lane i takes parts i, i + 64, ..., then the butterfly).
__global__ __launch_bounds__(256) void seg_calib_final_kernel(const float* __restrict__ wsf, float* __restrict__ sums, int64_t nparts) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int q = wave; q < SEG_CALIB_SUMS; q += 4) {
    float a = 0.f;
    for (int64_t p = lane; p < nparts; p += 64) a += wsf[p * SEG_CALIB_SUMS + q];
    a = wave_sum(a);
    if (lane == 0) sums[q] = a;
  }
}

static int64_t seg_calib_parts(int64_t B, int g) { return ceil_div(B * g * g, (int64_t)SEG_CALIB_CELLS); }

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
extern "C" int64_t dinox_seg_calib_ws_bytes(int64_t B, int g, int u, int C, int NB) {
  if (seg_broken_limit(B, g, u, C) || !(NB >= 1 && NB <= SEG_CALIB_MAX_BINS)) return 0;
  return seg_calib_parts(B, g) * SEG_CALIB_SUMS * (int64_t)sizeof(float);
}

extern "C" int dinox_seg_calib(const float* z, const uint8_t* y, float inv_temperature, uint8_t* pred, float* conf, float* entropy, int64_t* hist,
                               float* sums, void* ws, int64_t B, int g, int u, int C, int NB, void* stream) {
  int rc = seg_geometry("seg_calib", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(NB >= 1 && NB <= SEG_CALIB_MAX_BINS, DINOX_EINVAL, "seg_calib: NB=%d bins (1 <= NB <= %d)", NB, SEG_CALIB_MAX_BINS);
  DX_REQUIRE(inv_temperature > 0.f && std::isfinite(inv_temperature), DINOX_EINVAL, "seg_calib: inv_temperature=%g (finite and > 0)",
             (double)inv_temperature);
  DX_REQUIRE(z, DINOX_EINVAL, "seg_calib: null pointer (z)");
  if (y)
    DX_REQUIRE(hist && sums && ws, DINOX_EINVAL, "seg_calib: labels come with hist, sums and ws (all four or none)");
  else
    DX_REQUIRE(!hist && !sums && !ws, DINOX_EINVAL, "seg_calib: hist, sums and ws come with labels (all four or none)");
  DX_REQUIRE(y || pred || conf || entropy, DINOX_EINVAL, "seg_calib: nothing to compute (no labels and no output map)");
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g;
  if (hist) {
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)(3 * NB + 3) * sizeof(int64_t), st);
    if (e != hipSuccess) return fail((int)e, "seg_calib: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  // without labels there is nothing to sum: a wave per cell, as dinox_seg_predict runs
  const int per = y ? SEG_CALIB_CELLS : 1;
  const int64_t parts = ceil_div(ncell, (int64_t)per);
  const unsigned grid = (unsigned)ceil_div(parts, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u), inv_logc = 1.0f / logf((float)C);
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_calib_kernel<decltype(cp)::value>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, inv_temperature, inv_logc, pred, conf,
                       entropy, (unsigned long long*)hist, (float*)ws, g, u, C, NB, inv2u, y ? seg_wide(y, u) : 0, pred ? seg_wide(pred, u) : 0, ncell,
                       per, parts);
  });
  rc = check_launch("seg_calib");
  if (rc || !y) return rc;
  hipLaunchKernelGGL(seg_calib_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, sums, parts);
  return check_launch("seg_calib (sum)");
}
