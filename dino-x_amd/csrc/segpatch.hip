// segpatch.hip -- patch sampling for segmentation training at native resolution: one launch turns B jobs into the image batch
// x [B][3][S][S] and the label batch m [B][S][S], both read from a device-resident pool of planes under the job's inverse affine map
// (image bilinear with constant padding, gamma, gain and normalisation; label nearest with 255 outside).  Definitions: include/dinox.h.
//
// Layout.  A WAVE takes a run of 64 consecutive output pixels of one row, as segblend.hip does, so the job index is wave-uniform: the
// job's four integers and eight parameters are read at uniform addresses, the row coordinate dy and the two products with it are
// uniform, and each lane computes its source coordinates ONCE for both outputs.  A lane then reads one label byte and four image taps
// (a gather: consecutive lanes read neighbouring source pixels under any matrix near the identity, a rotated or mirrored row walks the
// plane at a slant), and stores one float per channel and one byte: the stores of a run are contiguous.  No LDS, no atomics, no sum
// that crosses lanes: equal inputs give equal bytes.
// Addresses: a coordinate is compared with the plane's bounds IN FLOAT (a NaN fails every comparison, a huge value fails one) before
// it is converted to an integer, and every tap index is tested against [0, W) / [0, H) before it is used: no content of par can move a
// load outside the job's own plane.  The planes themselves come from jobs, which the kernel trusts (the caller checks its host copy).
#include "small_common.h"

namespace dinox {

constexpr int SP_WAVES = 4;                       // waves (= 64-pixel runs) per workgroup

struct SpNorm {
  float mean[3], std[3];
};

__global__ __launch_bounds__(64 * SP_WAVES) void seg_patch_sample_kernel(const float* __restrict__ img, const uint8_t* __restrict__ msk,
                                                                         const int64_t* __restrict__ jobs, const float* __restrict__ par,
                                                                         float* __restrict__ x, uint8_t* __restrict__ m, int S, float half, int nxr,
                                                                         int64_t nrun, float pad, SpNorm nrm, int mwide) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int64_t run = (int64_t)blockIdx.x * SP_WAVES + wave;
  if (run >= nrun) return;                        // uniform; nothing below synchronises the workgroup
  const int xr = (int)(run % nxr), oy = (int)((run / nxr) % S);
  const int64_t b = run / ((int64_t)nxr * S);
  const int64_t* job = jobs + 4 * b;
  const float* p = par + 8 * b;
  const float* ip = img + job[0];
  const uint8_t* mp = msk + job[1];
  const int H = (int)job[2], W = (int)job[3];     // (host: 1 <= H, W <= 2^20, so both are exact in fp32)
  const float Hf = (float)H, Wf = (float)W;
  const float a00 = p[0], a01 = p[1], a02 = p[2], a10 = p[3], a11 = p[4], a12 = p[5], gamma = p[6], gain = p[7];
  const int ox = xr * 64 + lane;
  const bool ok = ox < S;
  // the source point of the pixel's centre: exact dx, dy, then the two fma chains of the contract
  const float dx = (float)ox + 0.5f - half, dy = (float)oy + 0.5f - half;
  const float sx = fmaf(a00, dx, fmaf(a01, dy, a02)), sy = fmaf(a10, dx, fmaf(a11, dy, a12));

  // label: the source pixel that contains the point
  unsigned lab = 255u;
  if (sx >= 0.f && sx < Wf && sy >= 0.f && sy < Hf) {
    const int ix = (int)sx, iy = (int)sy;
    if (ok && (unsigned)ix < (unsigned)W && (unsigned)iy < (unsigned)H) lab = mp[(int64_t)iy * W + ix];
  }

  // image: bilinear between pixel centres; a tap outside the plane is `pad`
  const float u = sx - 0.5f, v = sy - 0.5f;
  float val = pad;
  if (u > -1.f && u < Wf && v > -1.f && v < Hf) {
    const float fu = floorf(u), fv = floorf(v);
    const int x0 = (int)fu, y0 = (int)fv, x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = u - fu, wy1 = v - fv, wx0 = 1.f - wx1, wy0 = 1.f - wy1;
    const bool cx0 = (unsigned)x0 < (unsigned)W, cx1 = (unsigned)x1 < (unsigned)W;
    const bool cy0 = ok && (unsigned)y0 < (unsigned)H, cy1 = ok && (unsigned)y1 < (unsigned)H;
    const float v00 = (cy0 && cx0) ? ip[(int64_t)y0 * W + x0] : pad;
    const float v01 = (cy0 && cx1) ? ip[(int64_t)y0 * W + x1] : pad;
    const float v10 = (cy1 && cx0) ? ip[(int64_t)y1 * W + x0] : pad;
    const float v11 = (cy1 && cx1) ? ip[(int64_t)y1 * W + x1] : pad;
    val = wy0 * (wx0 * v00 + wx1 * v01) + wy1 * (wx0 * v10 + wx1 * v11);
  }
  if (gamma != 1.f) val = powf(fmaxf(val, 0.f), gamma);          // uniform branch: the identity job stays exact
  val = gain * val;

  const int64_t pix = (b * S + oy) * (int64_t)S + ox;
  if (ok) {
    float* xo = x + (b * 3 * S + oy) * (int64_t)S + ox;
    const int64_t plane = (int64_t)S * S;
    xo[0] = (val - nrm.mean[0]) / nrm.std[0];
    xo[plane] = (val - nrm.mean[1]) / nrm.std[1];
    xo[2 * plane] = (val - nrm.mean[2]) / nrm.std[2];
  }
  if (mwide) {                                    // S % 4 == 0 and m 4-byte aligned: four lanes' bytes leave as one 32-bit store
    unsigned w = lab << (8 * (lane & 3));
    w |= __shfl_xor(w, 1, 64);
    w |= __shfl_xor(w, 2, 64);
    if (ok && (lane & 3) == 0) *reinterpret_cast<unsigned*>(m + pix) = w;
  } else if (ok) {
    m[pix] = (uint8_t)lab;
  }
}

}  // namespace dinox

using namespace dinox;

extern "C" int dinox_seg_patch_sample(const float* img, const uint8_t* msk, const int64_t* jobs, const float* par, float* x, uint8_t* m, int64_t B,
                                      int S, const float* mean, const float* stdev, float pad, void* stream) {
  DX_REQUIRE(img && msk && jobs && par && x && m && mean && stdev, DINOX_EINVAL, "seg_patch_sample: null pointer");
  DX_REQUIRE(S >= 1 && S <= (1 << 14), DINOX_EINVAL, "seg_patch_sample: S=%d (1 <= S <= 2^14)", S);
  DX_REQUIRE(B >= 1 && B <= (1 << 20), DINOX_EINVAL, "seg_patch_sample: B=%lld (1 <= B <= 2^20)", (long long)B);
  const int nxr = (int)ceil_div(S, 64);
  const int64_t nrun = B * S * nxr;
  DX_REQUIRE(nrun <= ((int64_t)1 << 31), DINOX_EINVAL, "seg_patch_sample: B S ceil(S / 64) = %lld runs (at most 2^31)", (long long)nrun);
  SpNorm nrm;
  for (int c = 0; c < 3; ++c) {
    DX_REQUIRE(std::isfinite(mean[c]) && std::isfinite(stdev[c]) && stdev[c] > 0.f, DINOX_EINVAL,
               "seg_patch_sample: mean[%d]=%g std[%d]=%g (finite, std > 0)", c, (double)mean[c], c, (double)stdev[c]);
    nrm.mean[c] = mean[c];
    nrm.std[c] = stdev[c];
  }
  DX_REQUIRE(std::isfinite(pad), DINOX_EINVAL, "seg_patch_sample: pad=%g is not finite", (double)pad);
  const unsigned grid = (unsigned)ceil_div(nrun, (int64_t)SP_WAVES);
  const int mwide = S % 4 == 0 && (reinterpret_cast<uintptr_t>(m) & 3) == 0;
  hipLaunchKernelGGL(seg_patch_sample_kernel, dim3(grid), dim3(64 * SP_WAVES), 0, as_stream(stream), img, msk, jobs, par, x, m, S, 0.5f * (float)S, nxr,
                     nrun, pad, nrm, mwide);
  return check_launch("seg_patch_sample");
}
