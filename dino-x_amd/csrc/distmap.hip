// distmap.hip -- the dense signed Euclidean distance map of a label map, per (image, class), in the units of the spacing (definitions:
// include/dinox.h): phi_c(p) = +d(p, G) where p lies outside the class, -d(p, R) where it lies inside, G = {y = c}, R = the valid pixels of
// the other classes; 0 at ignored pixels and wherever the set a pixel needs is empty.  The exact separable transform of surfdist.hip
// (sentinels and side limit: surf_common.h), two launches:
//
//   1. dist_columns_kernel: a THREAD per column of one (image, class), lanes along x.  Two sweeps (down, then up over the thread's own
//      values) write per pixel the vertical distance in pixels to the nearest G pixel and to the nearest R pixel of its column: two uint16
//      planes, SURF_NONE where the column has none.
//   2. dist_rows_kernel: a WORKGROUP per (image, class, row).  Both rows of column distances go to LDS as (s_y d)^2; every valid pixel x
//      takes min over x' of (s_x (x - x'))^2 + the value of the plane its own membership selects (outside: G, inside: R), the correctly
//      rounded square root and the sign.  A thread keeps FOUR x in registers and reads four x' in one 16-byte LDS word that every lane of
//      the wave shares (a broadcast): 16 candidates per LDS instruction.  A plane is walked only if the row has a pixel that needs it and
//      the image a source in it, so a row of an absent or all-covering class costs its loads and one store.
//
// No floating-point atomics and no sums at all: every output is a function of its image's labels and spacing only -- equal inputs give
// equal bits, an image's planes do not depend on its batch-mates, nor a class's plane on the other classes beyond which pixels are valid.
// A distance is sqrt(fl(fl(fl(s_x k)^2) + fl(fl(s_y m)^2))) with contraction off and a correctly rounded square root: within 3 u of the
// exact one, relatively (u = 2^-24), as in surfdist.hip.  A label is compared with class numbers only; it never becomes an address.
#include "surf_common.h"

namespace dinox {

constexpr int DIST_NX = 4;                         // pixels of a row per thread of dist_rows_kernel

// ---------------------------------------------------------------- 1: the column scan
// col[(b C + c) 2 + k][H][W] uint16, k = 0: to the nearest G pixel, k = 1: to the nearest R pixel.  bad[0]: labels >= C other than 255
// (counted by the c = 0 threads).
__global__ __launch_bounds__(256) void dist_columns_kernel(const uint8_t* __restrict__ y, uint16_t* __restrict__ col, unsigned long long* __restrict__ bad,
                                                           int H, int W, int C, int nxb) {
  const int xb = (int)(blockIdx.x % nxb);
  const int64_t pc = blockIdx.x / nxb;              // b C + c
  const int c = (int)(pc % C);
  const int64_t b = pc / C;
  const int x = xb * 256 + (int)threadIdx.x;
  if (x >= W) return;                               // no barrier in this kernel
  const int64_t hw = (int64_t)H * W;
  const uint8_t* yb = y + b * hw + x;
  uint16_t* cg = col + pc * 2 * hw + x;
  uint16_t* cr = cg + hw;
  unsigned nbad = 0;
  int lastg = -1, lastr = -1;
  for (int r = 0; r < H; ++r) {
    const int v = yb[(int64_t)r * W];
    if (v == c) lastg = r;
    else if (v < C) lastr = r;                      // 255 (ignore) and every other value >= C: in neither set
    else if (v != 255) ++nbad;
    cg[(int64_t)r * W] = (uint16_t)(lastg < 0 ? SURF_NONE : (unsigned)(r - lastg));
    cr[(int64_t)r * W] = (uint16_t)(lastr < 0 ? SURF_NONE : (unsigned)(r - lastr));
  }
  lastg = lastr = -1;
  for (int r = H - 1; r >= 0; --r) {                // the thread's own stores: visible to it
    const unsigned vg = cg[(int64_t)r * W], vr = cr[(int64_t)r * W];
    if (vg == 0) lastg = r;
    if (vr == 0) lastr = r;
    const unsigned dg = lastg < 0 ? SURF_NONE : (unsigned)(lastg - r), dr = lastr < 0 ? SURF_NONE : (unsigned)(lastr - r);
    if (dg < vg) cg[(int64_t)r * W] = (uint16_t)dg;
    if (dr < vr) cr[(int64_t)r * W] = (uint16_t)dr;
  }
  if (c == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// ---------------------------------------------------------------- 2: the row minimum, the root and the sign
// m[j] = min over x' < W4 of fl(fl(s_x (x_j - x'))^2) + g2[x'] for the thread's DIST_NX pixels; g2 holds +inf from W up to W4.
__device__ __forceinline__ void dist_row_min(const float* g2, const float (&xf)[DIST_NX], float sx, int W4, float (&m)[DIST_NX]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < DIST_NX; ++j) m[j] = __uint_as_float(SURF_INF);
  for (int xo = 0; xo < W4; xo += 4) {
    const float4 q = *reinterpret_cast<const float4*>(g2 + xo);
    const float gv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float xof = (float)(xo + k);
#pragma unroll
      for (int j = 0; j < DIST_NX; ++j) {
        const float dx = sx * (xf[j] - xof);        // the difference of two integers below 2^24: exact
        m[j] = fminf(m[j], dx * dx + gv[k]);
      }
    }
  }
}

// phi[(b C + c)][H][W] fp32.  W <= THREADS * DIST_NX <= SURF_MAX_SIDE: thread t keeps the pixels t, t + THREADS, ...
template <int THREADS>
__global__ __launch_bounds__(THREADS) void dist_rows_kernel(const uint8_t* __restrict__ y, const uint16_t* __restrict__ col, const float* __restrict__ spacing,
                                                            float* __restrict__ phi, int H, int W, int C) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float g2[2][THREADS * DIST_NX];   // W4 <= THREADS DIST_NX <= SURF_MAX_SIDE
  __shared__ unsigned flags;                        // 1: a pixel of G in this row, 2: one of R, 4: a G source in the image, 8: an R source
  const int tid = (int)threadIdx.x;
  const int row = (int)(blockIdx.x % H);
  const int64_t pc = blockIdx.x / H;                // b C + c
  const int c = (int)(pc % C);
  const int64_t b = pc / C;
  const int64_t hw = (int64_t)H * W;
  const uint8_t* yr = y + b * hw + (int64_t)row * W;
  const uint16_t* cg = col + pc * 2 * hw + (int64_t)row * W;
  const uint16_t* cr = cg + hw;
  float* out = phi + pc * hw + (int64_t)row * W;
  const float sy = spacing[2 * b], sx = spacing[2 * b + 1];
  const int W4 = (W + 3) & ~3;                      // <= THREADS DIST_NX, a multiple of 4 itself
  if (tid == 0) flags = 0;
  int side[DIST_NX];                                // +1: in R, the distance to G counts; -1: in G; 0: ignored, or no pixel
  float xf[DIST_NX];
  unsigned f = 0;
#pragma unroll
  for (int j = 0; j < DIST_NX; ++j) {
    const int x = j * THREADS + tid;
    const int v = x < W ? yr[x] : 255;
    side[j] = v == c ? -1 : (v < C ? 1 : 0);
    xf[j] = (float)x;
    f |= v == c ? 1u : (v < C ? 2u : 0u);
  }
  for (int x = tid; x < W4; x += THREADS) {
    const unsigned vg = x < W ? cg[x] : SURF_NONE, vr = x < W ? cr[x] : SURF_NONE;
    const float tg = sy * (float)vg, tr = sy * (float)vr;
    g2[0][x] = vg == SURF_NONE ? __uint_as_float(SURF_INF) : tg * tg;
    g2[1][x] = vr == SURF_NONE ? __uint_as_float(SURF_INF) : tr * tr;
    f |= (vg != SURF_NONE ? 4u : 0u) | (vr != SURF_NONE ? 8u : 0u);   // a column of this row has a source: the image has one
  }
  __syncthreads();                                  // flags = 0 is visible
  if (f) atomicOr(&flags, f);
  __syncthreads();                                  // flags and both LDS rows are complete
  const unsigned all = flags;
  float r[DIST_NX], m[DIST_NX];
#pragma unroll
  for (int j = 0; j < DIST_NX; ++j) r[j] = 0.f;
  if ((all & 2u) && (all & 4u)) {                   // uniform: pixels outside the class, and a G pixel to measure to
    dist_row_min(g2[0], xf, sx, W4, m);
#pragma unroll
    for (int j = 0; j < DIST_NX; ++j)
      if (side[j] > 0) r[j] = sqrtf(m[j]);          // correctly rounded (the compiler's default for fp32 sqrt)
  }
  if ((all & 1u) && (all & 8u)) {                   // uniform: pixels of the class, and an R pixel to measure to
    dist_row_min(g2[1], xf, sx, W4, m);
#pragma unroll
    for (int j = 0; j < DIST_NX; ++j)
      if (side[j] < 0) r[j] = -sqrtf(m[j]);
  }
#pragma unroll
  for (int j = 0; j < DIST_NX; ++j) {
    const int x = j * THREADS + tid;
    if (x < W) out[x] = r[j];
  }
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// B C H workgroups (the row launch) stay inside 2^30 and every plane index inside int64.
static bool distance_sizes_ok(int64_t B, int H, int W, int C) {
  return B >= 1 && B <= (1 << 20) && H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE && C >= 2 && C <= SEG_MAX_CLASSES &&
         B * C * H <= ((int64_t)1 << 30);
}

extern "C" size_t dinox_signed_distance_ws_bytes(int64_t B, int H, int W, int C) {
  return distance_sizes_ok(B, H, W, C) ? (size_t)(B * C * 2 * (int64_t)H * W * (int64_t)sizeof(uint16_t)) : 0;
}

extern "C" int dinox_signed_distance(const uint8_t* y, const float* spacing, float* phi, int64_t* bad, void* ws, int64_t B, int H, int W, int C,
                                     void* stream) {
  DX_REQUIRE(y && spacing && phi && bad && ws, DINOX_EINVAL, "signed_distance: null pointer");
  DX_REQUIRE(H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE, DINOX_EINVAL, "signed_distance: H=%d W=%d (1 <= H, W <= %d)", H, W,
             SURF_MAX_SIDE);
  DX_REQUIRE(C >= 2, DINOX_EINVAL, "signed_distance: C=%d (2 <= C <= %d)", C, SEG_MAX_CLASSES);
  DX_REQUIRE(C <= SEG_MAX_CLASSES, DINOX_EUNSUPPORTED, "signed_distance: C=%d classes: at most %d, as the segmentation loss takes", C, SEG_MAX_CLASSES);
  DX_REQUIRE(distance_sizes_ok(B, H, W, C), DINOX_EINVAL, "signed_distance: B=%lld (B >= 1 and B C H <= 2^30; map a longer batch in pieces)",
             (long long)B);
  hipStream_t st = as_stream(stream);
  const int64_t planes = B * C;
  uint16_t* col = (uint16_t*)ws;
  const hipError_t e = hipMemsetAsync(bad, 0, sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "signed_distance: hipMemsetAsync: %s", hipGetErrorString(e));
  const int nxb = (int)ceil_div(W, 256);
  hipLaunchKernelGGL(dist_columns_kernel, dim3((unsigned)(planes * nxb)), dim3(256), 0, st, y, col, (unsigned long long*)bad, H, W, C, nxb);
  const int rc = check_launch("signed_distance (columns)");
  if (rc) return rc;
  if (W <= 64 * DIST_NX)                            // one wave covers the row: no thread without a pixel to keep at 224
    hipLaunchKernelGGL((dist_rows_kernel<64>), dim3((unsigned)(planes * H)), dim3(64), 0, st, y, col, spacing, phi, H, W, C);
  else
    hipLaunchKernelGGL((dist_rows_kernel<256>), dim3((unsigned)(planes * H)), dim3(256), 0, st, y, col, spacing, phi, H, W, C);
  return check_launch("signed_distance (rows)");
}
