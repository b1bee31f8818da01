// encode_prep.hip -- device-side preprocessing of the inference surface (zoo.encode): source element -> fp32 -> HU (format) ->
// window -> PIL bilinear resize to S x S -> ImageNet normalise, in ONE kernel writing the fp32 [B][3][S][S] batch PatchViT.forward
// takes.  Restates the reference's zoo/encode.py:34-72,129-157 (NumPy + three PIL resizes per image on the host).
//
// The resize is PIL's Image.BILINEAR on a mode-F image (ImagingResample, precompute_coeffs): separable, horizontal pass first with
// an fp32 intermediate; along an axis of n -> S pixels: scale = n / S, fs = max(scale, 1), support = fs; per output index i:
// centre = (i + .5) scale, taps [max(int(centre - support + .5), 0), min(int(centre + support + .5), n)), weight of tap x =
// max(0, 1 - |(x - centre + .5) / fs|), renormalised to sum 1.  PIL computes the weights in double: so does this kernel (32 lanes, a
// handful of taps each), then keeps them in fp32; the sums run in fp32 (PIL: double, rounded to fp32 per pass).  At n == S the
// weights are exactly 1 and 0 and the resize is the identity to the bit.
//
// Unit of work: a PLANE JOB, not an image channel.  jobs[j] = {element offset of the plane in src, H, W, row stride, pixel stride,
// number of destinations (1..3), three destination indices image * 3 + channel}.  The plane is staged and filtered ONCE and the
// result leaves to every destination with that channel's mean / std: an (H, W) image (which the reference replicates) is one job
// with three destinations, a volume costs one resize per plane although every plane shows in three 2.5D stacks.
//
// One workgroup per 16 x 16 output tile of one job, as views.hip: the windowed footprint of the tile (at most 16 scale + 2 support
// + 2 pixels a side) is staged in LDS, filtered horizontally into a [rows][16] strip, then vertically.  HBM-bound by design: every
// source pixel is read ~(1 + 2 support / (16 scale))^2 times (1.27x at 512 -> 224), from L2 after the first touch; each output is
// written once.  A tile whose footprint or tap count exceeds the tables is written as NaN: never silently wrong.
#include "common.h"

namespace dinox {

constexpr int EP_T = 16;          // output tile side
constexpr int EP_THREADS = 256;
constexpr int EP_JOB = 9;         // int64 fields per job
constexpr size_t EP_LDS_LIMIT = 150 * 1024;

template <typename T>
__global__ __launch_bounds__(EP_THREADS) void encode_prep_kernel(const T* __restrict__ src, const int64_t* __restrict__ jobs,
                                                               float* __restrict__ out, int n_images, int S, int tiles, int F, int MAXT,
                                                               float lo, float hi, float den, int fmt) {
  extern __shared__ float ep_smem[];
  float* stage = ep_smem;                // [F][F]   windowed footprint
  float* strip = stage + F * F;          // [F][16]  after the horizontal pass
  float* wx = strip + F * EP_T;          // [16][MAXT]
  float* wy = wx + EP_T * MAXT;          // [16][MAXT]
  __shared__ int s_min[2][EP_T], s_n[2][EP_T];

  const int ty = blockIdx.x / tiles, tx = blockIdx.x % tiles;
  const int64_t* p = jobs + (int64_t)blockIdx.y * EP_JOB;
  const int64_t off = p[0], rs = p[3], ps = p[4];
  const int H = (int)p[1], W = (int)p[2], nd = (int)p[5];
  const int ox0 = tx * EP_T, oy0 = ty * EP_T;

  // per output column / row of the tile: tap range and normalised weights
  const int t = threadIdx.x;
  if (t < 2 * EP_T) {
    const int axis = t / EP_T, q = t % EP_T;
    const int o = (axis == 0 ? ox0 : oy0) + q, n = axis == 0 ? W : H;
    int xmin = 0, xn = 0;
    float* w = (axis == 0 ? wx : wy) + q * MAXT;
    if (o < S && n > 0) {
      const double scale = (double)n / (double)S, fs = scale > 1.0 ? scale : 1.0;
      const double center = ((double)o + 0.5) * scale;
      xmin = max((int)(center - fs + 0.5), 0);
      xn = min((int)(center + fs + 0.5), n) - xmin;
      if (xn > MAXT || xn <= 0) xn = -1;                       // table too small for this plane (the host sizes it): poison the tile
      double tot = 0.0;
      for (int k = 0; k < xn; ++k) tot += fmax(0.0, 1.0 - fabs(((double)(k + xmin) - center + 0.5) / fs));
      for (int k = 0; k < xn; ++k) w[k] = (float)(fmax(0.0, 1.0 - fabs(((double)(k + xmin) - center + 0.5) / fs)) / tot);
    } else if (o < S) {
      xn = -1;
    }
    s_min[axis][q] = xmin;
    s_n[axis][q] = xn;
  }
  __syncthreads();
  // footprint of the tile in plane coordinates
  int fx0 = 0x7fffffff, fx1 = 0, fy0 = 0x7fffffff, fy1 = 0;
  bool bad = nd < 1 || nd > 3;
#pragma unroll
  for (int q = 0; q < EP_T; ++q) {
    if (ox0 + q < S) {
      bad |= s_n[0][q] < 0;
      fx0 = min(fx0, s_min[0][q]);
      fx1 = max(fx1, s_min[0][q] + s_n[0][q]);
    }
    if (oy0 + q < S) {
      bad |= s_n[1][q] < 0;
      fy0 = min(fy0, s_min[1][q]);
      fy1 = max(fy1, s_min[1][q] + s_n[1][q]);
    }
  }
  const int fw = fx1 - fx0, fh = fy1 - fy0;
  bad |= fw > F || fh > F;
  const int qy = t / EP_T, qx = t % EP_T;
  const int oy = oy0 + qy, ox = ox0 + qx;
  float a = __builtin_nanf("");
  if (!bad) {
    // stage the footprint: element -> fp32 -> HU -> window (reference zoo/encode.py:34-63; true division)
    const T* plane = src + off;
    for (int e = t; e < fh * fw; e += EP_THREADS) {
      const int ry = e / fw, rx = e % fw;
      float x = (float)plane[(int64_t)(fy0 + ry) * rs + (int64_t)(fx0 + rx) * ps];
      if (fmt == DINOX_FMT_HU16_PNG) x = (x - 32768.0f) * 0.1f;
      if (fmt != DINOX_FMT_WINDOWED_FLOAT) {
        x = x < lo ? lo : (x > hi ? hi : x);                     // np.clip: a NaN stays a NaN
        x = (x - lo) / den;
      }
      stage[ry * F + rx] = x;
    }
    __syncthreads();
    // horizontal pass: strip[ry][q] = sum_k wx[q][k] * stage[ry][xmin_q - fx0 + k]
    for (int e = t; e < fh * EP_T; e += EP_THREADS) {
      const int ry = e / EP_T, q = e % EP_T;
      float h = 0.f;
      if (ox0 + q < S) {
        const float* s = stage + ry * F + (s_min[0][q] - fx0);
        const float* w = wx + q * MAXT;
        const int n = s_n[0][q];
        for (int k = 0; k < n; ++k) h += w[k] * s[k];
      }
      strip[ry * EP_T + q] = h;
    }
    __syncthreads();
    // vertical pass
    if (oy < S && ox < S) {
      const float* w = wy + qy * MAXT;
      const int n = s_n[1][qy], r0 = s_min[1][qy] - fy0;
      a = 0.f;
      for (int k = 0; k < n; ++k) a += w[k] * strip[(r0 + k) * EP_T + qx];
    }
  }
  // one result, up to three (image, channel) destinations, each with its own normalisation
  if (oy < S && ox < S) {
    const int nw = bad ? 3 : nd;                                 // (a poisoned tile reaches every slot that names a destination)
    for (int d = 0; d < nw; ++d) {
      const int64_t dst = p[6 + d];
      if (dst < 0 || dst >= (int64_t)n_images * 3) continue;     // a destination index never becomes an address outside out
      const int c = (int)(dst % 3);
      const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
      const float stdv = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
      out[(dst * S + oy) * (int64_t)S + ox] = (a - mean) / stdv;
    }
  }
}

static void ep_tables(int S, int max_side, int& F, int& MAXT) {
  const double s = (double)max_side / (double)S, sup = s > 1.0 ? s : 1.0;
  F = (int)(EP_T * s + 2.0 * sup) + 4;
  MAXT = (int)(2.0 * sup) + 3;
}

template <typename T>
static int launch_encode_prep(const void* src, const int64_t* jobs, int n_jobs, float* out, int n_images, int S, int F, int MAXT, size_t lds,
                              float lo, float hi, float den, int fmt, void* stream) {
  if (int rc = reserve_lds(reinterpret_cast<const void*>(encode_prep_kernel<T>), lds, "encode_preprocess")) return rc;
  const int tiles = (S + EP_T - 1) / EP_T;
  hipLaunchKernelGGL(encode_prep_kernel<T>, dim3((unsigned)(tiles * tiles), (unsigned)n_jobs), dim3(EP_THREADS), lds, as_stream(stream),
                     (const T*)src, jobs, out, n_images, S, tiles, F, MAXT, lo, hi, den, fmt);
  return check_launch("encode_preprocess");
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_encode_preprocess_lds_bytes(int S, int max_side) {
  if (S <= 0 || max_side <= 0) return -1;
  const double s = (double)max_side / (double)S, sup = s > 1.0 ? s : 1.0;
  const int64_t F = (int64_t)(EP_T * s + 2.0 * sup) + 4, MAXT = (int64_t)(2.0 * sup) + 3;
  return (F * F + F * EP_T + 2 * EP_T * MAXT) * (int64_t)sizeof(float);
}

extern "C" int dinox_encode_preprocess(const void* src, int src_dtype, const int64_t* jobs, int n_jobs, float* out, int n_images, int S,
                                       int max_side, double lo, double hi, int format, void* stream) {
  DX_REQUIRE(src && jobs && out, DINOX_EINVAL, "encode_preprocess: null pointer");
  DX_REQUIRE(n_jobs > 0 && n_jobs <= 65535 && n_images > 0 && S > 0 && S <= 16384 && max_side > 0, DINOX_EINVAL,
             "encode_preprocess: n_jobs=%d n_images=%d S=%d max_side=%d", n_jobs, n_images, S, max_side);
  DX_REQUIRE(format == DINOX_FMT_HU_FLOAT || format == DINOX_FMT_HU16_PNG || format == DINOX_FMT_WINDOWED_FLOAT, DINOX_EINVAL,
             "encode_preprocess: format %d", format);
  DX_REQUIRE(src_dtype == DINOX_F32 || src_dtype == DINOX_U16 || src_dtype == DINOX_I16, DINOX_EINVAL, "encode_preprocess: source dtype %d",
             src_dtype);
  const int64_t need = dinox_encode_preprocess_lds_bytes(S, max_side);
  DX_REQUIRE(need <= (int64_t)EP_LDS_LIMIT, DINOX_EUNSUPPORTED, "encode_preprocess: a %d-pixel side down to %d needs %lld B of LDS (limit 150 KiB)",
             max_side, S, (long long)need);
  int F, MAXT;
  ep_tables(S, max_side, F, MAXT);
  // the window bounds as the reference's NumPy sees them: lo, hi and hi - lo are Python doubles that meet an fp32 array
  const float flo = (float)lo, fhi = (float)hi, den = (float)(hi - lo);
  const size_t lds = (size_t)need;
  if (src_dtype == DINOX_U16) return launch_encode_prep<uint16_t>(src, jobs, n_jobs, out, n_images, S, F, MAXT, lds, flo, fhi, den, format, stream);
  if (src_dtype == DINOX_I16) return launch_encode_prep<int16_t>(src, jobs, n_jobs, out, n_images, S, F, MAXT, lds, flo, fhi, den, format, stream);
  return launch_encode_prep<float>(src, jobs, n_jobs, out, n_images, S, F, MAXT, lds, flo, fhi, den, format, stream);
}
