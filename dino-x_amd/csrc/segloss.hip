// segloss.hip -- dense segmentation loss on patch logits: bilinear upsampling (align_corners = False), softmax, cross-entropy and soft Dice,
// their gradient, and the arg-max prediction, without a full-resolution logit tensor in memory in either direction (definitions:
// include/dinox.h).
//
// Layout.  The S x S pixels of an image fall into g x g CELLS: cell (cy, cx) holds the pixels whose upper-left tap is patch (cy, cx), i.e.
// rows [lo(cy), lo(cy + 1)) and columns [lo(cx), lo(cx + 1)) with lo(0) = 0, lo(k) = k u + u / 2, lo(g) = S.  Every pixel of a cell
// interpolates the same four patches, so a WAVE takes a cell: it reads the four logit rows once (wave-uniform addresses), a lane keeps one
// pixel column (its x weights fold the rows into two C-vectors in registers) and walks down the cell's rows, 64 / width rows per step.
// Per pixel the C logits, the softmax and every per-class term live in registers.  A cell is at most 48 x 48 pixels (u <= 32).
// Sums: a lane adds its pixels in row order, the wave adds its lanes by the xor butterfly, partial sums go to the workspace with plain
// stores and a second launch adds them in ascending order -- no floating-point atomics anywhere.  The label and prediction COUNTS are
// integers and use integer atomics (LDS; global for dinox_seg_predict's int64 counts).
// A label is compared with class numbers and 255 only; it never becomes an address beyond a [0, C) slot of an LDS counter.
#include "small_common.h"
#include "kernels.h"
#include "seg_common.h"

namespace dinox {

// SEG_WAVES, the cell walk seg_cell_pixels and seg_softmax: seg_common.h (csrc/segcalib.hip walks the same cells)
constexpr int SEG_FWD_CELLS = 8;                  // cells per partial sum of dinox_seg_loss_fwd

// What the boundary-term variants of the kernels below take beyond the others (BD = false: nothing, and those instantiations compile to
// what they were before the term existed).  phi[B][C][S][S]: the signed distance maps of csrc/distmap.hip.
template <bool BD>
struct SegBd {};
template <>
struct SegBd<true> {
  const float* phi;
  int c0;
  float w_bd;
  int only_bd;                                    // seg_fwd_final_kernel writes loss[3] alone
};

// ---------------------------------------------------------------- forward: partial sums of SEG_FWD_CELLS cells per wave
// wsf[part][1 + 2 C] = (sum of lse - l_y, P[C], I[C]); wsi[part][C + 2] = (Y[C], valid pixels, labels outside [0, C) other than 255).
// BD (the boundary term, dinox_seg_loss_bd_fwd): wsf[part][2 + 2 C], the last float the sum of p_pc phi_c(p) over the valid pixels and c >= c0,
// phi read at the pixel the lane holds (coalesced along x, the planes below c0 not at all).
template <int CP, bool BD = false>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_fwd_partial_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, float* __restrict__ wsf,
                                                                         unsigned* __restrict__ wsi, int g, int u, int C, float inv2u, int ywide,
                                                                         int64_t ncell, int64_t nparts, SegBd<BD> bdp) {
  __shared__ unsigned cnt[SEG_WAVES][CP + 2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t part = (int64_t)blockIdx.x * SEG_WAVES + wave;
  for (int i = lane; i < CP + 2; i += 64) cnt[wave][i] = 0;
  __syncthreads();
  float P[CP], I[CP], ce = 0.f;
  [[maybe_unused]] float bd = 0.f;
#pragma unroll
  for (int c = 0; c < CP; ++c) P[c] = I[c] = 0.f;
  if (part < nparts) {
    const int64_t c_end = (part + 1) * SEG_FWD_CELLS < ncell ? (part + 1) * SEG_FWD_CELLS : ncell;
    for (int64_t cell = part * SEG_FWD_CELLS; cell < c_end; ++cell) {
      [[maybe_unused]] const int64_t ss = (int64_t)(g * u) * (g * u);
      [[maybe_unused]] const float* pb = nullptr;
      if constexpr (BD) pb = bdp.phi + (cell / ((int64_t)g * g)) * C * ss;
      seg_cell_pixels<CP>(z, y, g, u, C, inv2u, ywide, cell, lane, [&](bool ok, int lab, float, float, float(&l)[CP], int Y, int X) {
        if (!ok || lab == 255) return;
        if (lab >= C) {
          atomicAdd(&cnt[wave][CP + 1], 1u);
          return;
        }
        float ly = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) ly = lab == c ? l[c] : ly;
        float m, sum;
        seg_softmax<CP>(l, C, m, sum);
        ce += (logf(sum) + m) - ly;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
          P[c] += l[c];
          I[c] += lab == c ? l[c] : 0.f;
        }
        if constexpr (BD) {
          const float* pp = pb + (int64_t)Y * (g * u) + X;
#pragma unroll
          for (int c = 0; c < CP; ++c)
            if (c >= bdp.c0 && c < C) bd += l[c] * pp[c * ss];
        }
        atomicAdd(&cnt[wave][lab], 1u);
        atomicAdd(&cnt[wave][CP], 1u);
      });
    }
  }
  ce = wave_sum(ce);
  if constexpr (BD) bd = wave_sum(bd);
  float outP = 0.f, outI = 0.f;                   // lane c keeps class c's sums: one coalesced store each
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    const float p = wave_sum(P[c]), i = wave_sum(I[c]);
    if (lane == c) outP = p, outI = i;
  }
  __syncthreads();                                // the LDS counters of every wave are complete
  if (part < nparts) {
    float* wf = wsf + part * (1 + 2 * C + (BD ? 1 : 0));
    unsigned* wi = wsi + part * (C + 2);
    if (lane == 0) wf[0] = ce;
    if (lane < C) {
      wf[1 + lane] = outP;
      wf[1 + C + lane] = outI;
      wi[lane] = cnt[wave][lane];
    }
    if (lane == 0) wi[C] = cnt[wave][CP], wi[C + 1] = cnt[wave][CP + 1];
    if constexpr (BD)
      if (lane == 0) wf[1 + 2 * C] = bd;
  }
}

// One workgroup: the partial sums in a fixed order (lane i takes parts i, i + 64, ..., then the butterfly), then the losses.
// BD: one float more per part (above); loss[3] = its sum / (Nv (C - c0)), and w_bd times that joins L.  only_bd: nothing but loss[3] is
// written (the other outputs are then those of the kernels without the term, dinox_seg_loss_bd_fwd with w_bd = 0).
template <bool BD = false>
__global__ __launch_bounds__(256) void seg_fwd_final_kernel(const float* __restrict__ wsf, const unsigned* __restrict__ wsi, float* __restrict__ loss,
                                                            float* __restrict__ stats, int64_t* __restrict__ nv, int C, int c0, float w_ce,
                                                            float w_dice, int64_t nparts, SegBd<BD> bdp) {
  __shared__ float sf[1 + 2 * 64 + (BD ? 1 : 0)];
  __shared__ double si[64 + 2];
  __shared__ float dc[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nf = 1 + 2 * C + (BD ? 1 : 0), ni = C + 2;
  for (int q = wave; q < nf + ni; q += 4) {
    if (q < nf) {
      float a = 0.f;
      for (int64_t p = lane; p < nparts; p += 64) a += wsf[p * nf + q];
      a = wave_sum(a);
      if (lane == 0) sf[q] = a;
    } else {
      double a = 0.0;                             // counts: exact in double
      for (int64_t p = lane; p < nparts; p += 64) a += (double)wsi[p * ni + (q - nf)];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (lane == 0) si[q - nf] = a;
    }
  }
  __syncthreads();
  const double nvd = si[C];
  const int c = threadIdx.x;
  if constexpr (BD) {
    if (bdp.only_bd) {                            // uniform
      if (threadIdx.x == 0) loss[3] = nvd > 0 ? sf[1 + 2 * C] / ((float)nvd * (float)(C - c0)) : 0.f;
      return;
    }
  }
  if (c < C) {
    const float Pc = sf[1 + c], Ic = sf[1 + C + c], Yc = (float)si[c];
    stats[c] = nvd > 0 ? Ic : 0.f;
    stats[C + c] = nvd > 0 ? Pc : 0.f;
    stats[2 * C + c] = Yc;
    dc[c] = (2.f * Ic + 1.f) / ((Pc + Yc) + 1.f);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nv[0] = (int64_t)nvd;
    nv[1] = (int64_t)si[C + 1];
    float ce = 0.f, dice = 0.f;
    if (nvd > 0) {
      ce = sf[0] / (float)nvd;
      float d = 0.f;
      for (int k = c0; k < C; ++k) d += dc[k];
      dice = 1.f - d / (float)(C - c0);
    }
    float L = w_ce * ce + w_dice * dice;
    if constexpr (BD) {
      const float bd = nvd > 0 ? sf[1 + 2 * C] / ((float)nvd * (float)(C - c0)) : 0.f;
      L += bdp.w_bd * bd;
      loss[3] = bd;
    }
    loss[0] = L;
    loss[1] = ce;
    loss[2] = dice;
  }
}

// ---------------------------------------------------------------- backward: per cell, the four taps' sums of W(p, tap) G_p
// wsb[cell][4][C]: tap (ty, tx) at index 2 ty + tx; a clamped second tap carries weight 0 (its weight went to the first).
// BD: the boundary term's G_pc += kbd p_pc (phi_pc - sum_k p_pk phi_pk), kbd = w_bd / (Nv (C - c0)), has the Dice term's shape and is added
// in the same pixel pass, after the same softmax, as a term of its own beside the other two.
template <int CP, bool BD = false>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_bwd_cells_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y,
                                                                       const float* __restrict__ stats, const int64_t* __restrict__ nv,
                                                                       float* __restrict__ wsb, int g, int u, int C, int c0, float w_ce, float w_dice,
                                                                       float inv2u, int ywide, int64_t ncell, SegBd<BD> bdp) {
  __shared__ float al[CP], be[CP];                // w_dice a_pc = be[c] + [y_p = c] al[c]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x < CP) {
    const int c = threadIdx.x;
    float a = 0.f, bt = 0.f;
    if (c >= c0 && c < C) {
      const float k = w_dice / (float)(C - c0);
      const float den = (stats[C + c] + stats[2 * C + c]) + 1.f, num = 2.f * stats[c] + 1.f;
      a = -2.f * k / den;
      bt = k * num / (den * den);
    }
    al[c] = a;
    be[c] = bt;
  }
  __syncthreads();
  const int64_t cell = (int64_t)blockIdx.x * SEG_WAVES + wave;
  if (cell >= ncell) return;                      // no barrier below
  const int64_t nvv = nv[0];
  const float kce = nvv > 0 ? w_ce / (float)nvv : 0.f;
  [[maybe_unused]] float kbd = 0.f;
  [[maybe_unused]] const int64_t ss = (int64_t)(g * u) * (g * u);
  [[maybe_unused]] const float* pb = nullptr;
  if constexpr (BD) {
    kbd = nvv > 0 ? bdp.w_bd / ((float)nvv * (float)(C - c0)) : 0.f;
    pb = bdp.phi + (cell / ((int64_t)g * g)) * C * ss;
  }
  float T0[CP], T1[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) T0[c] = T1[c] = 0.f;
  seg_cell_pixels<CP>(z, y, g, u, C, inv2u, ywide, cell, lane, [&](bool ok, int lab, float wy0, float wy1, float(&l)[CP], int Y, int X) {
    if (!ok || lab >= C) return;
    float m, sum;
    seg_softmax<CP>(l, C, m, sum);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) dot += l[c] * (be[c] + (lab == c ? al[c] : 0.f));
    [[maybe_unused]] float t[CP], dotb = 0.f;     // BD: t = kbd phi_pc and sum_k p_pk t_k
    if constexpr (BD) {
      const float* pp = pb + (int64_t)Y * (g * u) + X;
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        t[c] = c >= c0 && c < C ? kbd * pp[c * ss] : 0.f;
        dotb += l[c] * t[c];
      }
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const bool hit = lab == c;
      float G = kce * (l[c] - (hit ? 1.f : 0.f)) + l[c] * ((be[c] + (hit ? al[c] : 0.f)) - dot);
      if constexpr (BD) G += l[c] * (t[c] - dotb);
      T0[c] += wy0 * G;
      T1[c] += wy1 * G;
    }
  });
  const int cx = (int)(cell % g);
  const float wx1 = seg_w1(seg_lane_x(cx, g, u, lane), cx, g, u, inv2u), wx0 = 1.f - wx1;      // the lane's column weights, as in seg_cell_pixels
  float out[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    if (c < C) {                                  // uniform
      const float s00 = wave_sum(wx0 * T0[c]), s01 = wave_sum(wx1 * T0[c]), s10 = wave_sum(wx0 * T1[c]), s11 = wave_sum(wx1 * T1[c]);
      if (lane == c) out[0] = s00, out[1] = s01, out[2] = s10, out[3] = s11;
    }
  }
  if (lane < C) {
    float* w = wsb + cell * 4 * C;
#pragma unroll
    for (int t = 0; t < 4; ++t) w[t * C + lane] = out[t];
  }
}

// dz[b][jy][jx][c] = gscale (t00(jy, jx) + t01(jy, jx - 1) + t10(jy - 1, jx) + t11(jy - 1, jx - 1)), absent cells left out, in that order.
__global__ __launch_bounds__(256) void seg_bwd_gather_kernel(const float* __restrict__ wsb, float* __restrict__ dz, float gscale, int g, int C,
                                                             int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const int64_t cell = i / C;
  const int jx = (int)(cell % g), jy = (int)((cell / g) % g);
  float a = wsb[cell * 4 * C + c];
  if (jx > 0) a += wsb[(cell - 1) * 4 * C + C + c];
  if (jy > 0) a += wsb[(cell - g) * 4 * C + 2 * C + c];
  if (jx > 0 && jy > 0) a += wsb[(cell - g - 1) * 4 * C + 3 * C + c];
  dz[i] = gscale * a;
}

// ---------------------------------------------------------------- predict: arg-max label map and the confusion counts
template <int CP>
__global__ __launch_bounds__(64 * SEG_WAVES) void seg_predict_kernel(const float* __restrict__ z, const uint8_t* __restrict__ y, uint8_t* __restrict__ pred,
                                                                     unsigned long long* __restrict__ counts, int g, int u, int C, float inv2u,
                                                                     int ywide, int pwide, int64_t ncell) {
  __shared__ unsigned cnt[SEG_WAVES][3 * CP + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, S = g * u;
  const int64_t cell = (int64_t)blockIdx.x * SEG_WAVES + wave;
  for (int i = lane; i < 3 * CP + 1; i += 64) cnt[wave][i] = 0;
  __syncthreads();
  if (cell < ncell) {
    uint8_t* pb = pred + (cell / ((int64_t)g * g)) * (int64_t)S * S;
    seg_cell_pixels<CP>(z, y, g, u, C, inv2u, ywide, cell, lane, [&](bool ok, int lab, float, float, float(&l)[CP], int Y, int X) {
      int best = 0;
      float bv = l[0];
#pragma unroll
      for (int c = 1; c < CP; ++c)
        if (c < C && l[c] > bv) bv = l[c], best = c;
      if (pwide) {                                // four lanes' bytes leave as one 32-bit store
        unsigned w = (unsigned)best << (8 * (lane & 3));
        w |= __shfl_xor(w, 1, 64);
        w |= __shfl_xor(w, 2, 64);
        if (ok && (lane & 3) == 0) *reinterpret_cast<unsigned*>(pb + (int64_t)Y * S + X) = w;
      } else if (ok) {
        pb[(int64_t)Y * S + X] = (uint8_t)best;
      }
      if (!ok || lab == 255) return;
      if (lab >= C) {
        atomicAdd(&cnt[wave][3 * CP], 1u);
        return;
      }
      if (best == lab) atomicAdd(&cnt[wave][best], 1u);
      atomicAdd(&cnt[wave][CP + best], 1u);
      atomicAdd(&cnt[wave][2 * CP + lab], 1u);
    });
  }
  __syncthreads();
  if (cell < ncell && counts) {
    if (lane < C)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (cnt[wave][t * CP + lane]) atomicAdd(&counts[t * C + lane], (unsigned long long)cnt[wave][t * CP + lane]);
    if (lane == 0 && cnt[wave][3 * CP]) atomicAdd(&counts[3 * C], (unsigned long long)cnt[wave][3 * CP]);
  }
}

// ---------------------------------------------------------------- host
// seg_cp / seg_by_width (the register width that holds C classes), seg_wide, seg_broken_limit / seg_geometry (the size limits): seg_common.h

static int64_t seg_fwd_parts(int64_t B, int g) { return ceil_div(B * g * g, (int64_t)SEG_FWD_CELLS); }

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
extern "C" int64_t dinox_seg_loss_ws_bytes(int64_t B, int g, int u, int C) {
  if (seg_broken_limit(B, g, u, C)) return 0;
  const int64_t ncell = B * g * g, parts = seg_fwd_parts(B, g);
  const int64_t fwd = parts * (1 + 2 * C) * 4 + parts * (C + 2) * 4, bwd = ncell * 4 * C * 4;
  return fwd > bwd ? fwd : bwd;
}

extern "C" int dinox_seg_loss_fwd(const float* z, const uint8_t* y, float* loss, float* stats, int64_t* nv, void* ws, int64_t B, int g, int u, int C,
                                  int c0, float w_ce, float w_dice, void* stream) {
  DX_REQUIRE(z && y && loss && stats && nv && ws, DINOX_EINVAL, "seg_loss_fwd: null pointer");
  int rc = seg_geometry("seg_loss_fwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_fwd: c0=%d (0: every class in the Dice term, 1: without class 0)", c0);
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g, parts = seg_fwd_parts(B, g);
  float* wsf = (float*)ws;
  unsigned* wsi = (unsigned*)(wsf + parts * (1 + 2 * C));
  const unsigned grid = (unsigned)ceil_div(parts, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u);
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_fwd_partial_kernel<decltype(cp)::value>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, wsf, wsi, g, u, C, inv2u,
                       seg_wide(y, u), ncell, parts, SegBd<false>{});
  });
  rc = check_launch("seg_loss_fwd (partials)");
  if (rc) return rc;
  hipLaunchKernelGGL(seg_fwd_final_kernel<false>, dim3(1), dim3(256), 0, st, wsf, wsi, loss, stats, nv, C, c0, w_ce, w_dice, parts, SegBd<false>{});
  return check_launch("seg_loss_fwd (sum)");
}

extern "C" int dinox_seg_loss_bwd(const float* z, const uint8_t* y, const float* stats, const int64_t* nv, float* dz, void* ws, int64_t B, int g,
                                  int u, int C, int c0, float w_ce, float w_dice, float grad_scale, void* stream) {
  DX_REQUIRE(z && y && stats && nv && dz && ws, DINOX_EINVAL, "seg_loss_bwd: null pointer");
  int rc = seg_geometry("seg_loss_bwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_bwd: c0=%d (0: every class in the Dice term, 1: without class 0)", c0);
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g;
  float* wsb = (float*)ws;
  const unsigned grid = (unsigned)ceil_div(ncell, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u);
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_bwd_cells_kernel<decltype(cp)::value>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, stats, nv, wsb, g, u, C, c0, w_ce,
                       w_dice, inv2u, seg_wide(y, u), ncell, SegBd<false>{});
  });
  rc = check_launch("seg_loss_bwd (cells)");
  if (rc) return rc;
  const int64_t total = ncell * C;
  hipLaunchKernelGGL(seg_bwd_gather_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, wsb, dz, grad_scale, g, C, total);
  return check_launch("seg_loss_bwd (gather)");
}

// ---------------------------------------------------------------- the same with the boundary term (phi: csrc/distmap.hip)
extern "C" size_t dinox_seg_loss_bd_ws_bytes(int64_t B, int g, int u, int C) {
  if (seg_broken_limit(B, g, u, C)) return 0;
  const int64_t ncell = B * g * g, parts = seg_fwd_parts(B, g);
  const int64_t fwd = parts * (2 + 2 * C) * 4 + parts * (C + 2) * 4, bwd = ncell * 4 * C * 4;
  return (size_t)(fwd > bwd ? fwd : bwd);
}

extern "C" int dinox_seg_loss_bd_fwd(const float* z, const uint8_t* y, const float* phi, float* loss, float* stats, int64_t* nv, void* ws, int64_t B,
                                     int g, int u, int C, int c0, float w_ce, float w_dice, float w_bd, void* stream) {
  DX_REQUIRE(z && y && phi && loss && stats && nv && ws, DINOX_EINVAL, "seg_loss_bd_fwd: null pointer");
  int rc = seg_geometry("seg_loss_bd_fwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_bd_fwd: c0=%d (0: every class in the Dice and boundary terms, 1: without class 0)", c0);
  // w_bd = 0 promises the bits of dinox_seg_loss_fwd.  How the compiler fuses the shared sums differs between the two instantiations (seen
  // at C > 32: P_c accumulated by a fused multiply-add in one, a multiply and an add in the other), so that promise is kept by running
  // those very kernels; the boundary kernels then report BD alone, in the one case where nothing trains on it.
  const bool only_bd = w_bd == 0.f;
  if (only_bd) {
    rc = dinox_seg_loss_fwd(z, y, loss, stats, nv, ws, B, g, u, C, c0, w_ce, w_dice, stream);
    if (rc) return rc;
  }
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g, parts = seg_fwd_parts(B, g);
  float* wsf = (float*)ws;
  unsigned* wsi = (unsigned*)(wsf + parts * (2 + 2 * C));
  const unsigned grid = (unsigned)ceil_div(parts, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u);
  const SegBd<true> bdp{phi, c0, w_bd, only_bd ? 1 : 0};
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_fwd_partial_kernel<decltype(cp)::value, true>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, wsf, wsi, g, u, C, inv2u,
                       seg_wide(y, u), ncell, parts, bdp);
  });
  rc = check_launch("seg_loss_bd_fwd (partials)");
  if (rc) return rc;
  hipLaunchKernelGGL(seg_fwd_final_kernel<true>, dim3(1), dim3(256), 0, st, wsf, wsi, loss, stats, nv, C, c0, w_ce, w_dice, parts, bdp);
  return check_launch("seg_loss_bd_fwd (sum)");
}

extern "C" int dinox_seg_loss_bd_bwd(const float* z, const uint8_t* y, const float* phi, const float* stats, const int64_t* nv, float* dz, void* ws,
                                     int64_t B, int g, int u, int C, int c0, float w_ce, float w_dice, float w_bd, float grad_scale, void* stream) {
  DX_REQUIRE(z && y && phi && stats && nv && dz && ws, DINOX_EINVAL, "seg_loss_bd_bwd: null pointer");
  int rc = seg_geometry("seg_loss_bd_bwd", B, g, u, C);
  if (rc) return rc;
  DX_REQUIRE(c0 == 0 || c0 == 1, DINOX_EINVAL, "seg_loss_bd_bwd: c0=%d (0: every class in the Dice and boundary terms, 1: without class 0)", c0);
  if (w_bd == 0.f)                                // the gradient has no boundary term: the kernels without it, and their bits (see the forward)
    return dinox_seg_loss_bwd(z, y, stats, nv, dz, ws, B, g, u, C, c0, w_ce, w_dice, grad_scale, stream);
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g;
  float* wsb = (float*)ws;
  const unsigned grid = (unsigned)ceil_div(ncell, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u);
  const SegBd<true> bdp{phi, c0, w_bd, 0};
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_bwd_cells_kernel<decltype(cp)::value, true>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, stats, nv, wsb, g, u, C, c0,
                       w_ce, w_dice, inv2u, seg_wide(y, u), ncell, bdp);
  });
  rc = check_launch("seg_loss_bd_bwd (cells)");
  if (rc) return rc;
  const int64_t total = ncell * C;
  hipLaunchKernelGGL(seg_bwd_gather_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, st, wsb, dz, grad_scale, g, C, total);
  return check_launch("seg_loss_bd_bwd (gather)");
}

extern "C" int dinox_seg_predict(const float* z, const uint8_t* y, uint8_t* pred, int64_t* counts, int64_t B, int g, int u, int C, void* stream) {
  DX_REQUIRE(z && pred, DINOX_EINVAL, "seg_predict: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "seg_predict: labels and counts come together (both or neither)");
  const int rc = seg_geometry("seg_predict", B, g, u, C);
  if (rc) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t ncell = B * g * g;
  if (counts) {
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)(3 * C + 1) * sizeof(int64_t), st);
    if (e != hipSuccess) return fail((int)e, "seg_predict: hipMemsetAsync: %s", hipGetErrorString(e));
  }
  const unsigned grid = (unsigned)ceil_div(ncell, (int64_t)SEG_WAVES);
  const float inv2u = 1.0f / (float)(2 * u);
  seg_by_width(C, [&](auto cp) {
    hipLaunchKernelGGL((seg_predict_kernel<decltype(cp)::value>), dim3(grid), dim3(64 * SEG_WAVES), 0, st, z, y, pred, (unsigned long long*)counts, g, u,
                       C, inv2u, y ? seg_wide(y, u) : 0, seg_wide(pred, u), ncell);
  });
  return check_launch("seg_predict");
}
