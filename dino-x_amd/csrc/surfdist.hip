// surfdist.hip -- surface distances between two label maps in mm: per (image, class, direction) the number of border pixels, the sum, the
// maximum and a nearest-rank quantile of their distances to the other map's border, and the number within each tolerance (definitions:
// include/dinox.h).  An exact separable Euclidean distance transform, three launches:
//
//   1. surf_columns_kernel: a THREAD per column of one (image, plane in {pred, gt}, class), lanes along x.  It reads the label maps as
//      they are (no one-hot planes), decides border membership from the four edge neighbours and writes per pixel the vertical distance in
//      pixels to the nearest border pixel of its column as uint16 (0 = this pixel is a border pixel, SURF_NONE = none in this column):
//      a sweep down, then a sweep up over the thread's own values.
//   2. surf_rows_kernel: a WORKGROUP per (image, class, direction, row).  The other plane's row of column distances goes to LDS as
//      (s_y d)^2; every border pixel x of the query plane takes min over x' of (s_x (x - x'))^2 + that value and its square root.  Every
//      lane of a wave reads the same LDS word (a broadcast).  Non-border pixels get SURF_SKIP; rows without a border pixel leave early.
//   3. surf_reduce_kernel: a WORKGROUP per (image, class, direction) reads its plane of distances (it sits in L2): count, sum (per lane in
//      ascending order, wave butterfly, per-wave partials in ascending order), maximum and tolerance counts (integers), then the k-th
//      smallest by a radix select on the bit patterns of the non-negative fp32 distances -- four 8-bit digit histograms in LDS.
//
// No floating-point atomics, no sort, no host round trip; equal inputs give equal bits, and an image's results do not depend on what
// else is in the batch.  A label is compared with class numbers and 255 only; it never becomes an address.
// A distance is sqrt(fl(fl(fl(s_x k)^2) + fl(fl(s_y m)^2))) with contraction off and a correctly rounded square root: within 3 u of the
// exact one, relatively (u = 2^-24).
#include "surf_common.h"

namespace dinox {

// p is in the set of (plane, c) (surf_member).  Outside the image: not in the set.
__device__ __forceinline__ bool surf_in(const uint8_t* __restrict__ pb, const uint8_t* __restrict__ gb, int plane, int c, int H, int W, int y, int x) {
  if (y < 0 || y >= H || x < 0 || x >= W) return false;
  return surf_member(pb, gb, (int64_t)y * W + x, plane, c);
}

// ---------------------------------------------------------------- 1: border membership and the column scan
// col[((b 2 + plane) C + c)][H][W] uint16.  bad[0] / bad[1]: pred values >= C / gt values >= C other than 255 (counted by the c = 0 threads).
__global__ __launch_bounds__(256) void surf_columns_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, uint16_t* __restrict__ col,
                                                           unsigned long long* __restrict__ bad, int H, int W, int C, int nxb) {
  const int xb = (int)(blockIdx.x % nxb);
  const int64_t img = blockIdx.x / nxb;             // (b 2 + plane) C + c
  const int c = (int)(img % C), plane = (int)((img / C) % 2);
  const int64_t b = img / (2 * (int64_t)C);
  const int x = xb * 256 + (int)threadIdx.x;
  if (x >= W) return;                               // no barrier in this kernel
  const int64_t hw = (int64_t)H * W;
  const uint8_t* pb = pred + b * hw;
  const uint8_t* gb = gt + b * hw;
  uint16_t* cd = col + img * hw + x;
  unsigned nbad = 0;
  int last = -1;
  bool up = false, cur = surf_in(pb, gb, plane, c, H, W, 0, x);
  for (int y = 0; y < H; ++y) {
    const bool down = surf_in(pb, gb, plane, c, H, W, y + 1, x);
    const bool border = cur && !(up && down && surf_in(pb, gb, plane, c, H, W, y, x - 1) && surf_in(pb, gb, plane, c, H, W, y, x + 1));
    if (c == 0) {
      const int v = plane == 0 ? pb[(int64_t)y * W + x] : gb[(int64_t)y * W + x];
      nbad += surf_bad_label(v, plane, C) ? 1u : 0u;
    }
    if (border) last = y;
    cd[(int64_t)y * W] = (uint16_t)(last < 0 ? SURF_NONE : (unsigned)(y - last));
    up = cur;
    cur = down;
  }
  last = -1;
  for (int y = H - 1; y >= 0; --y) {                // the thread's own stores: visible to it
    const unsigned v = cd[(int64_t)y * W];
    if (v == 0) last = y;
    const unsigned d = last < 0 ? SURF_NONE : (unsigned)(last - y);
    if (d < v) cd[(int64_t)y * W] = (uint16_t)d;
  }
  if (nbad) atomicAdd(&bad[plane], (unsigned long long)nbad);
}

// ---------------------------------------------------------------- 2: the row minimum
// dist[((b C + c) 2 + dir)][H][W] fp32; dir 0: from the border of pred to the border of gt, dir 1: the other way.
__global__ __launch_bounds__(256) void surf_rows_kernel(const uint16_t* __restrict__ col, const float* __restrict__ spacing, float* __restrict__ dist, int H,
                                                        int W, int C) {
#pragma clang fp contract(off)
  __shared__ float g2[SURF_MAX_SIDE];
  const int y = (int)(blockIdx.x % H);
  const int64_t plane_id = blockIdx.x / H;          // (b C + c) 2 + dir
  const int dir = (int)(plane_id % 2), c = (int)((plane_id / 2) % C);
  const int64_t b = plane_id / (2 * (int64_t)C);
  const int64_t hw = (int64_t)H * W;
  const uint16_t* own = col + ((b * 2 + dir) * C + c) * hw + (int64_t)y * W;
  const uint16_t* oth = col + ((b * 2 + (1 - dir)) * C + c) * hw + (int64_t)y * W;
  float* out = dist + plane_id * hw + (int64_t)y * W;
  const float sy = spacing[2 * b], sx = spacing[2 * b + 1];
  bool query[SURF_MAX_SIDE / 256];
  int any = 0;
#pragma unroll
  for (int j = 0; j < SURF_MAX_SIDE / 256; ++j) {
    const int x = j * 256 + (int)threadIdx.x;
    query[j] = x < W && own[x] == 0;
    any |= query[j] ? 1 : 0;
  }
  if (!__syncthreads_or(any)) {                     // uniform: no border pixel of the query side in this row
    for (int x = threadIdx.x; x < W; x += 256) out[x] = SURF_SKIP;
    return;
  }
  for (int x = threadIdx.x; x < W; x += 256) {
    const unsigned v = oth[x];
    const float t = sy * (float)v;
    g2[x] = v == SURF_NONE ? __uint_as_float(SURF_INF) : t * t;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SURF_MAX_SIDE / 256; ++j) {
    const int x = j * 256 + (int)threadIdx.x;
    if (x >= W) continue;
    float r = SURF_SKIP;
    if (query[j]) {
      float m = __uint_as_float(SURF_INF);
      for (int xo = 0; xo < W; ++xo) {
        const float dx = sx * (float)(x - xo);
        m = fminf(m, dx * dx + g2[xo]);
      }
      r = sqrtf(m);                                 // correctly rounded (the compiler's default for fp32 sqrt)
    }
    out[x] = r;
  }
}

// ---------------------------------------------------------------- 3: count, sum, maximum, tolerance counts and the k-th smallest
// counts[((b C + c) 2 + dir)][1 + T] int64 = (n, within tol_t); values[...][3] fp32 = (sum, max, quantile).
__global__ __launch_bounds__(256) void surf_reduce_kernel(const float* __restrict__ dist, int64_t* __restrict__ counts, float* __restrict__ values,
                                                          SurfTol tol, int64_t hw, int T, int q_num, int q_den) {
  __shared__ float red[16];
  __shared__ unsigned hist[256];
  __shared__ unsigned icnt[2 + SURF_MAX_TOL];       // n, max bits, within[T]
  __shared__ unsigned sel[2];                       // the prefix so far, the rank left inside it
  const int tid = threadIdx.x;
  const unsigned* d = reinterpret_cast<const unsigned*>(dist + (int64_t)blockIdx.x * hw);
  if (tid < 2 + SURF_MAX_TOL) icnt[tid] = 0;
  __syncthreads();
  float sum = 0.f;
  unsigned n = 0, mx = 0, within[SURF_MAX_TOL];
#pragma unroll
  for (int t = 0; t < SURF_MAX_TOL; ++t) within[t] = 0;
  for (int64_t i = tid; i < hw; i += 256) {
    const unsigned bits = d[i];
    if (bits >> 31) continue;
    const float v = __uint_as_float(bits);
    ++n;
    sum += v;
    mx = bits > mx ? bits : mx;                     // non-negative floats order as their bit patterns
#pragma unroll
    for (int t = 0; t < SURF_MAX_TOL; ++t) within[t] += (t < T && v <= tol.v[t]) ? 1u : 0u;
  }
  sum = block_sum(sum, red);
  if (n) {
    atomicAdd(&icnt[0], n);
    atomicMax(&icnt[1], mx);
#pragma unroll
    for (int t = 0; t < SURF_MAX_TOL; ++t)
      if (within[t]) atomicAdd(&icnt[2 + t], within[t]);
  }
  __syncthreads();
  const unsigned ntot = icnt[0], mxb = icnt[1];
  const bool empty = ntot == 0 || mxb == SURF_INF;  // no query border, or no border on the other side: the floats are 0
  int64_t* oc = counts + (int64_t)blockIdx.x * (1 + T);
  float* ov = values + (int64_t)blockIdx.x * 3;
  if (tid == 0) oc[0] = ntot;
  if (tid >= 1 && tid <= T) oc[tid] = empty ? 0 : (int64_t)icnt[1 + tid];
  if (empty) {
    if (tid < 3) ov[tid] = 0.f;
    return;                                         // uniform
  }
  // the k-th smallest, k = ceil(n q_num / q_den) in integers (1 <= k <= n)
  if (tid == 0) {
    sel[0] = 0;
    sel[1] = (unsigned)(((int64_t)ntot * q_num + q_den - 1) / q_den);
  }
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();                                // also publishes sel
    const unsigned prefix = sel[0];
    for (int64_t i = tid; i < hw; i += 256) {
      const unsigned bits = d[i];
      if (bits >> 31) continue;
      if (surf_radix_takes_part(bits, prefix, shift)) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned k = sel[1];
      const unsigned digit = surf_radix_pick(hist, k);
      sel[0] = prefix | (digit << shift);
      sel[1] = k;
    }
    __syncthreads();
  }
  if (tid == 0) {
    ov[0] = sum;
    ov[1] = __uint_as_float(mxb);
    ov[2] = __uint_as_float(sel[0]);
  }
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// B C 2 H workgroups (the row launch) stay inside 2^30 and every plane index inside int64.
static bool surface_sizes_ok(int64_t B, int H, int W, int C) {
  return B >= 1 && B <= (1 << 20) && H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE && C >= 2 && C <= SEG_MAX_CLASSES &&
         B * C * 2 * H <= ((int64_t)1 << 30);
}

extern "C" int64_t dinox_surface_ws_bytes(int64_t B, int H, int W, int C) {
  return surface_sizes_ok(B, H, W, C) ? B * C * 2 * (int64_t)H * W * (int64_t)(sizeof(uint16_t) + sizeof(float)) : 0;
}

extern "C" int dinox_surface_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values,
                                   int64_t* bad, void* ws, int64_t B, int H, int W, int C, int T, int q_num, int q_den, void* stream) {
  DX_REQUIRE(pred && gt && spacing && tol && counts && values && bad && ws, DINOX_EINVAL, "surface_stats: null pointer");
  DX_REQUIRE(H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE, DINOX_EINVAL, "surface_stats: H=%d W=%d (1 <= H, W <= %d)", H, W,
             SURF_MAX_SIDE);
  DX_REQUIRE(C >= 2 && C <= SEG_MAX_CLASSES, DINOX_EINVAL, "surface_stats: C=%d (2 <= C <= %d)", C, SEG_MAX_CLASSES);
  DX_REQUIRE(surface_sizes_ok(B, H, W, C), DINOX_EINVAL, "surface_stats: B=%lld (B >= 1 and B C 2 H <= 2^30; evaluate a longer batch in pieces)",
             (long long)B);
  DX_REQUIRE(T >= 1 && T <= SURF_MAX_TOL, DINOX_EINVAL, "surface_stats: T=%d tolerances (1 <= T <= %d)", T, SURF_MAX_TOL);
  for (int t = 0; t < T; ++t) DX_REQUIRE(tol[t] >= 0.f && tol[t] <= 3.0e38f, DINOX_EINVAL, "surface_stats: tolerance %d is %g (finite and >= 0)", t, (double)tol[t]);
  DX_REQUIRE(q_num > 0 && q_num <= q_den, DINOX_EINVAL, "surface_stats: quantile %d/%d (0 < q_num <= q_den)", q_num, q_den);
  hipStream_t st = as_stream(stream);
  const int64_t planes = B * C * 2, hw = (int64_t)H * W;
  uint16_t* col = (uint16_t*)ws;
  float* dist = (float*)(col + planes * hw);        // planes * hw * 2 bytes: a multiple of 4
  const hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "surface_stats: hipMemsetAsync: %s", hipGetErrorString(e));
  const int nxb = (int)ceil_div(W, 256);
  hipLaunchKernelGGL(surf_columns_kernel, dim3((unsigned)(planes * nxb)), dim3(256), 0, st, pred, gt, col, (unsigned long long*)bad, H, W, C, nxb);
  int rc = check_launch("surface_stats (columns)");
  if (rc) return rc;
  hipLaunchKernelGGL(surf_rows_kernel, dim3((unsigned)(planes * H)), dim3(256), 0, st, col, spacing, dist, H, W, C);
  rc = check_launch("surface_stats (rows)");
  if (rc) return rc;
  SurfTol tv;
  for (int t = 0; t < SURF_MAX_TOL; ++t) tv.v[t] = t < T ? tol[t] : 0.f;
  hipLaunchKernelGGL(surf_reduce_kernel, dim3((unsigned)planes), dim3(256), 0, st, dist, counts, values, tv, hw, T, q_num, q_den);
  return check_launch("surface_stats (reduce)");
}
