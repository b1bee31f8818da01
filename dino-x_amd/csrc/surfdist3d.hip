// surfdist3d.hip -- surface distances between two label VOLUMES [Z][H][W] in mm with the anisotropic voxel (s_z, s_y, s_x): per (class,
// direction) the number of border voxels, the sum, the maximum and a nearest-rank quantile of their distances to the other volume's
// border, and the number within each tolerance (definitions: include/dinox.h).  An exact separable Euclidean distance transform in three
// axis passes.  The entry walks the classes one at a time over the same planes, so the workspace does not grow with C.  Per class:
//
//   1. surf3d_z_kernel: a THREAD per (plane in {pred, gt}, y, x) column along z, lanes along x.  It reads the label volumes as they are
//      (no one-hot planes), decides border membership from the six face neighbours and writes per voxel the distance in voxels to the
//      nearest border voxel of its z column as uint16 (0 = this voxel is a border voxel, SURF_NONE = none in this column): a sweep down,
//      then a sweep up over the thread's own values.  The class-0 launch also counts the bad labels.
//   2. surf3d_y_kernel: a WORKGROUP per (plane, z, strip of 16 x).  The strip's columns go to LDS as (s_z d)^2 ([H][16] fp32, lanes with
//      consecutive x on consecutive banks, the four y of a wave on one broadcast word); every voxel of the strip, border or not, takes
//      min over y' of (s_y (y - y'))^2 + that value: the squared mm distance to the nearest border voxel of its (z, y)-plane column pair.
//      A thread keeps four y in registers per LDS read.
//   3. surf3d_x_kernel: a WORKGROUP per (z, y) line, both directions.  Both planes' lines of pass-2 values go to LDS; every border voxel
//      x of the query plane takes min over x' of (s_x (x - x'))^2 + the OTHER plane's value and its square root; every lane of a wave
//      reads the same LDS word (a broadcast).  The distance replaces the query plane's own pass-2 value in place (a thread overwrites only
//      what it staged itself, after the barrier); non-border voxels get SURF_SKIP; a line without a border voxel on either side leaves early.
//   4. surf3d_stats_kernel, a WORKGROUP per (slice, direction): count, maximum and tolerance counts (integers, integer atomics in global
//      memory), the slice's sum (per lane in ascending order, wave butterfly, per-wave partials in ascending order) and the first digit
//      histogram of the radix select.  Then surf3d_pick_kernel (one thread per direction picks the digit) and surf3d_hist_kernel (the next
//      digit's histogram over the slices) alternate for the other three digits, and surf3d_finish_kernel adds the slice sums in ascending
//      z in one workgroup, picks the last digit and writes the outputs.
//
// No floating-point atomics, no sort, no host round trip; equal inputs give equal bits whatever the workspace held.  A label is compared
// with class numbers and 255 only; it never becomes an address.
// A distance is sqrt(fl(fl(fl(s_x k)^2) + fl(fl(fl(s_y m)^2) + fl(fl(s_z n)^2)))) with contraction off and a correctly rounded square
// root: the radicand within (1 + u)^5 of the exact one, the root within 3.5 u relatively (u = 2^-24).
#include "surf_common.h"

namespace dinox {

#pragma clang fp contract(off)

constexpr int S3_XS = 16;                          // x columns per strip of the y pass: [1024][16] fp32 = 64 KiB of LDS at the largest H
constexpr int S3_YB = 4;                           // y per thread and LDS read in the y pass
constexpr int S3_YG = 256 / S3_XS;                 // y groups of a workgroup
static_assert((int64_t)SURF_MAX_SIDE * SURF_MAX_SIDE * SURF_MAX_SIDE <= ((int64_t)1 << 30), "Z H W <= 2^30: every count fits an unsigned 32-bit integer");

// state (uint32 words), zeroed on the stream before every class:
constexpr int S3_HIST = 0;                         // [2 directions][4 rounds][256] digit histograms
constexpr int S3_ICNT = 2 * 4 * 256;               // [2 directions][16]: n, max bits, within[8], prefix, rank left, 4 unused
constexpr int S3_STATE_WORDS = S3_ICNT + 2 * 16;
constexpr int S3_N = 0, S3_MAX = 1, S3_WITHIN = 2, S3_PREFIX = 10, S3_RANK = 11;

// ---------------------------------------------------------------- 1: border membership and the z scan
// zd[plane][Z][H][W] uint16.  bad[0] / bad[1]: pred values >= C / gt values >= C other than 255 (count_bad: the launch of class 0).
__global__ __launch_bounds__(256) void surf3d_z_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, uint16_t* __restrict__ zd,
                                                       unsigned long long* __restrict__ bad, int Z, int H, int W, int c, int C, int count_bad) {
  const int64_t hw = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int plane = (int)blockIdx.y;
  if (p >= hw) return;                              // no barrier in this kernel
  const int y = (int)(p / W), x = (int)(p % W);
  uint16_t* cd = zd + (int64_t)plane * Z * hw + p;
  unsigned nbad = 0;
  int last = -1;
  bool up = false, cur = surf_member(pred, gt, p, plane, c);
  for (int z = 0; z < Z; ++z) {
    const int64_t i = (int64_t)z * hw + p;
    const bool down = z + 1 < Z && surf_member(pred, gt, i + hw, plane, c);
    const bool border = cur && !(up && down && y > 0 && surf_member(pred, gt, i - W, plane, c) && y + 1 < H && surf_member(pred, gt, i + W, plane, c) &&
                                 x > 0 && surf_member(pred, gt, i - 1, plane, c) && x + 1 < W && surf_member(pred, gt, i + 1, plane, c));
    if (count_bad) nbad += surf_bad_label(plane == 0 ? pred[i] : gt[i], plane, C) ? 1u : 0u;
    if (border) last = z;
    cd[(int64_t)z * hw] = (uint16_t)(last < 0 ? SURF_NONE : (unsigned)(z - last));
    up = cur;
    cur = down;
  }
  last = -1;
  for (int z = Z - 1; z >= 0; --z) {                // the thread's own stores: visible to it
    const unsigned v = cd[(int64_t)z * hw];
    if (v == 0) last = z;
    const unsigned d = last < 0 ? SURF_NONE : (unsigned)(last - z);
    if (d < v) cd[(int64_t)z * hw] = (uint16_t)d;
  }
  if (nbad) atomicAdd(&bad[plane], (unsigned long long)nbad);
}

// ---------------------------------------------------------------- 2: the y minimum, at every voxel
// g[plane][Z][H][W] fp32 = min over y' of fl(fl(s_y (y - y'))^2) + fl(fl(s_z zd)^2), +inf where the (z, x) column pair holds no border voxel.
__global__ __launch_bounds__(256) void surf3d_y_kernel(const uint16_t* __restrict__ zd, float* __restrict__ g, float sz, float sy, int Z, int H, int W) {
  extern __shared__ float col[];                    // [H][S3_XS]
  const int xl = (int)threadIdx.x % S3_XS, yg = (int)threadIdx.x / S3_XS;
  const int x = (int)blockIdx.x * S3_XS + xl;
  const int64_t base = ((int64_t)blockIdx.z * Z + blockIdx.y) * H * W;
  for (int y = yg; y < H; y += S3_YG) {
    float v = __uint_as_float(SURF_INF);
    if (x < W) {
      const unsigned d = zd[base + (int64_t)y * W + x];
      const float t = sz * (float)d;
      if (d != SURF_NONE) v = t * t;
    }
    col[y * S3_XS + xl] = v;
  }
  __syncthreads();
  if (x >= W) return;                               // after the only barrier
  for (int yb = yg; yb < H; yb += S3_YG * S3_YB) {  // this thread's y: yb, yb + 16, yb + 32, yb + 48
    float m[S3_YB];
#pragma unroll
    for (int j = 0; j < S3_YB; ++j) m[j] = __uint_as_float(SURF_INF);
    for (int yo = 0; yo < H; ++yo) {
      const float cz = col[yo * S3_XS + xl];
#pragma unroll
      for (int j = 0; j < S3_YB; ++j) {
        const float dy = sy * (float)(yb + j * S3_YG - yo);
        m[j] = fminf(m[j], dy * dy + cz);
      }
    }
#pragma unroll
    for (int j = 0; j < S3_YB; ++j) {
      const int y = yb + j * S3_YG;
      if (y < H) g[base + (int64_t)y * W + x] = m[j];
    }
  }
}

// ---------------------------------------------------------------- 3: the x minimum at the query border voxels, in place
// g[dir][Z][H][W] becomes the distance plane of direction dir (0: from the border of pred to the border of gt; 1: the other way).
// No __restrict__ on g: a line is read and then overwritten.
__global__ __launch_bounds__(256) void surf3d_x_kernel(const uint16_t* __restrict__ zd, float* g, float sx, int64_t nvox, int W) {
  __shared__ float oth[2][SURF_MAX_SIDE];           // oth[dir]: the other plane's line
  const int64_t line = (int64_t)blockIdx.x * W;
  bool query[2][SURF_MAX_SIDE / 256];
  int any = 0;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir)
#pragma unroll
    for (int j = 0; j < SURF_MAX_SIDE / 256; ++j) {
      const int x = j * 256 + (int)threadIdx.x;
      query[dir][j] = x < W && zd[dir * nvox + line + x] == 0;
      any |= query[dir][j] ? (1 << dir) : 0;
    }
  any = (__syncthreads_or(any & 1) ? 1 : 0) | (__syncthreads_or(any & 2) ? 2 : 0);      // (the vote returns a truth value, not the OR) uniform from here on
  if (any) {
    for (int x = threadIdx.x; x < W; x += 256) {
      oth[0][x] = g[nvox + line + x];
      oth[1][x] = g[line + x];
    }
    __syncthreads();
  }
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    float* out = g + dir * nvox + line;
    if (!((any >> dir) & 1)) {                      // no border voxel of this query side on the line
      for (int x = threadIdx.x; x < W; x += 256) out[x] = SURF_SKIP;
      continue;
    }
#pragma unroll
    for (int j = 0; j < SURF_MAX_SIDE / 256; ++j) {
      const int x = j * 256 + (int)threadIdx.x;     // the x this thread staged: nobody else reads or writes g here
      if (x >= W) continue;
      float r = SURF_SKIP;
      if (query[dir][j]) {
        float m = __uint_as_float(SURF_INF);
        for (int xo = 0; xo < W; ++xo) {
          const float dx = sx * (float)(x - xo);
          m = fminf(m, dx * dx + oth[dir][xo]);
        }
        r = sqrtf(m);                               // correctly rounded (the compiler's default for fp32 sqrt)
      }
      out[x] = r;
    }
  }
}

// ---------------------------------------------------------------- 4: count, sum, maximum, tolerance counts and the k-th smallest
// One digit histogram of a slice, LDS first, then the occupied bins to global memory.  Every thread of the workgroup calls it.
__device__ __forceinline__ void surf3d_flush_hist(const unsigned* lds_hist, unsigned* hist) {
  __syncthreads();
  const unsigned v = lds_hist[threadIdx.x];
  if (v) atomicAdd(&hist[threadIdx.x], v);
}

// grid (Z, 2).  partial[dir][Z] fp32: the slice sums.
__global__ __launch_bounds__(256) void surf3d_stats_kernel(const float* __restrict__ dist, unsigned* __restrict__ state, float* __restrict__ partial, SurfTol tol,
                                                           int64_t hw, int64_t nvox, int T) {
  __shared__ float red[16];
  __shared__ unsigned hist[256];
  const int tid = threadIdx.x, z = blockIdx.x, dir = blockIdx.y, Z = gridDim.x;
  const unsigned* d = reinterpret_cast<const unsigned*>(dist + dir * nvox + (int64_t)z * hw);
  hist[tid] = 0;
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
    atomicAdd(&hist[bits >> 24], 1u);
  }
  sum = block_sum(sum, red);
  if (tid == 0) partial[dir * Z + z] = sum;
  unsigned* ic = state + S3_ICNT + dir * 16;
  if (n) {
    atomicAdd(&ic[S3_N], n);
    atomicMax(&ic[S3_MAX], mx);
#pragma unroll
    for (int t = 0; t < SURF_MAX_TOL; ++t)
      if (within[t]) atomicAdd(&ic[S3_WITHIN + t], within[t]);
  }
  surf3d_flush_hist(hist, state + S3_HIST + (dir * 4 + 0) * 256);
}

// The digit of `round` (0: bits 31..24) from its finished histogram: two threads, one per direction.  Round 0 also forms the rank
// k = ceil(n q_num / q_den) in integers (1 <= k <= n for n >= 1; n <= 2^30 and q_num < 2^31 keep the product inside int64).
__device__ __forceinline__ void surf3d_pick(unsigned* state, int dir, int round, int q_num, int q_den) {
  unsigned* ic = state + S3_ICNT + dir * 16;
  unsigned k = round == 0 ? (unsigned)(((int64_t)ic[S3_N] * q_num + q_den - 1) / q_den) : ic[S3_RANK];
  const unsigned digit = surf_radix_pick(state + S3_HIST + (dir * 4 + round) * 256, k);
  ic[S3_PREFIX] |= digit << (24 - 8 * round);
  ic[S3_RANK] = k;
}
__global__ __launch_bounds__(64) void surf3d_pick_kernel(unsigned* __restrict__ state, int round, int q_num, int q_den) {
  if (threadIdx.x < 2) surf3d_pick(state, (int)threadIdx.x, round, q_num, q_den);
}

// grid (Z, 2): the histogram of digit `round` (1, 2, 3) over the distances whose higher digits equal the prefix.
__global__ __launch_bounds__(256) void surf3d_hist_kernel(const float* __restrict__ dist, unsigned* __restrict__ state, int64_t hw, int64_t nvox, int round) {
  __shared__ unsigned hist[256];
  const int tid = threadIdx.x, z = blockIdx.x, dir = blockIdx.y, shift = 24 - 8 * round;
  const unsigned* d = reinterpret_cast<const unsigned*>(dist + dir * nvox + (int64_t)z * hw);
  const unsigned prefix = state[S3_ICNT + dir * 16 + S3_PREFIX];
  hist[tid] = 0;
  __syncthreads();
  for (int64_t i = tid; i < hw; i += 256) {
    const unsigned bits = d[i];
    if (bits >> 31) continue;
    if (surf_radix_takes_part(bits, prefix, shift)) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
  }
  surf3d_flush_hist(hist, state + S3_HIST + (dir * 4 + round) * 256);
}

// grid 2 (the direction).  counts[2][1 + T] int64 and values[2][3] fp32 of this class.
__global__ __launch_bounds__(256) void surf3d_finish_kernel(unsigned* __restrict__ state, const float* __restrict__ partial, int64_t* __restrict__ counts,
                                                            float* __restrict__ values, int Z, int T, int q_num, int q_den) {
  __shared__ float red[16];
  const int tid = threadIdx.x, dir = blockIdx.x;
  const float sum = block_strided_sum(partial + dir * Z, Z, red);      // ascending z per lane, then the fixed order of block_sum
  unsigned* ic = state + S3_ICNT + dir * 16;
  const unsigned ntot = ic[S3_N], mxb = ic[S3_MAX];
  const bool empty = ntot == 0 || mxb == SURF_INF;  // no query border, or no border on the other side: the floats are 0
  int64_t* oc = counts + (int64_t)dir * (1 + T);
  float* ov = values + (int64_t)dir * 3;
  if (tid == 0) oc[0] = ntot;
  if (tid >= 1 && tid <= T) oc[tid] = empty ? 0 : (int64_t)ic[S3_WITHIN + tid - 1];
  if (empty) {
    if (tid < 3) ov[tid] = 0.f;
    return;
  }
  if (tid == 0) {
    surf3d_pick(state, dir, 3, q_num, q_den);
    ov[0] = sum;
    ov[1] = __uint_as_float(mxb);
    ov[2] = __uint_as_float(ic[S3_PREFIX]);
  }
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
static bool surface3d_sizes_ok(int64_t Z, int H, int W, int C) {
  return Z >= 1 && Z <= SURF_MAX_SIDE && H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE && C >= 2 && C <= SEG_MAX_CLASSES;
}

// zd uint16 [2][Z][H][W], g fp32 [2][Z][H][W] (squared distances, then distances), partial fp32 [2][Z], state uint32 [S3_STATE_WORDS].
extern "C" int64_t dinox_surface3d_ws_bytes(int64_t Z, int H, int W, int C) {
  return surface3d_sizes_ok(Z, H, W, C) ? 12 * Z * H * W + 8 * Z + 4 * (int64_t)S3_STATE_WORDS : 0;
}

extern "C" int dinox_surface3d_stats(const uint8_t* pred, const uint8_t* gt, const float* spacing, const float* tol, int64_t* counts, float* values,
                                     int64_t* bad, void* ws, int64_t Z, int H, int W, int C, int T, int q_num, int q_den, void* stream) {
  DX_REQUIRE(pred && gt && spacing && tol && counts && values && bad && ws, DINOX_EINVAL, "surface3d_stats: null pointer");
  DX_REQUIRE(Z >= 1 && Z <= SURF_MAX_SIDE && H >= 1 && H <= SURF_MAX_SIDE && W >= 1 && W <= SURF_MAX_SIDE, DINOX_EINVAL,
             "surface3d_stats: Z=%lld H=%d W=%d (1 <= Z, H, W <= %d)", (long long)Z, H, W, SURF_MAX_SIDE);
  DX_REQUIRE(C >= 2 && C <= SEG_MAX_CLASSES, DINOX_EINVAL, "surface3d_stats: C=%d (2 <= C <= %d)", C, SEG_MAX_CLASSES);
  for (int a = 0; a < 3; ++a)
    DX_REQUIRE(spacing[a] > 0.f && spacing[a] <= 3.0e38f, DINOX_EINVAL, "surface3d_stats: spacing %d is %g (finite and > 0)", a, (double)spacing[a]);
  DX_REQUIRE(T >= 1 && T <= SURF_MAX_TOL, DINOX_EINVAL, "surface3d_stats: T=%d tolerances (1 <= T <= %d)", T, SURF_MAX_TOL);
  for (int t = 0; t < T; ++t)
    DX_REQUIRE(tol[t] >= 0.f && tol[t] <= 3.0e38f, DINOX_EINVAL, "surface3d_stats: tolerance %d is %g (finite and >= 0)", t, (double)tol[t]);
  DX_REQUIRE(q_num > 0 && q_num <= q_den, DINOX_EINVAL, "surface3d_stats: quantile %d/%d (0 < q_num <= q_den)", q_num, q_den);
  hipStream_t st = as_stream(stream);
  const int64_t hw = (int64_t)H * W, nvox = Z * hw;
  uint16_t* zd = (uint16_t*)ws;
  float* g = (float*)(zd + 2 * nvox);               // 4 nvox bytes: a multiple of 4
  float* partial = g + 2 * nvox;
  unsigned* state = (unsigned*)(partial + 2 * Z);
  hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int64_t), st);
  if (e != hipSuccess) return fail((int)e, "surface3d_stats: hipMemsetAsync: %s", hipGetErrorString(e));
  SurfTol tv;
  for (int t = 0; t < SURF_MAX_TOL; ++t) tv.v[t] = t < T ? tol[t] : 0.f;
  const float sz = spacing[0], sy = spacing[1], sx = spacing[2];
  const dim3 slices((unsigned)Z, 2);
  const size_t lds_y = (size_t)H * S3_XS * sizeof(float);            // at most 64 KiB
  for (int c = 0; c < C; ++c) {
    e = hipMemsetAsync(state, 0, S3_STATE_WORDS * sizeof(unsigned), st);
    if (e != hipSuccess) return fail((int)e, "surface3d_stats: hipMemsetAsync: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(surf3d_z_kernel, dim3((unsigned)ceil_div(hw, 256), 2), dim3(256), 0, st, pred, gt, zd, (unsigned long long*)bad, (int)Z, H, W, c, C,
                       c == 0 ? 1 : 0);
    int rc = check_launch("surface3d_stats (z)");
    if (rc) return rc;
    hipLaunchKernelGGL(surf3d_y_kernel, dim3((unsigned)ceil_div(W, S3_XS), (unsigned)Z, 2), dim3(256), lds_y, st, zd, g, sz, sy, (int)Z, H, W);
    rc = check_launch("surface3d_stats (y)");
    if (rc) return rc;
    hipLaunchKernelGGL(surf3d_x_kernel, dim3((unsigned)(Z * H)), dim3(256), 0, st, zd, g, sx, nvox, W);
    rc = check_launch("surface3d_stats (x)");
    if (rc) return rc;
    hipLaunchKernelGGL(surf3d_stats_kernel, slices, dim3(256), 0, st, g, state, partial, tv, hw, nvox, T);
    rc = check_launch("surface3d_stats (stats)");
    if (rc) return rc;
    for (int round = 0; round < 3; ++round) {
      hipLaunchKernelGGL(surf3d_pick_kernel, dim3(1), dim3(64), 0, st, state, round, q_num, q_den);
      rc = check_launch("surface3d_stats (pick)");
      if (rc) return rc;
      hipLaunchKernelGGL(surf3d_hist_kernel, slices, dim3(256), 0, st, g, state, hw, nvox, round + 1);
      rc = check_launch("surface3d_stats (histogram)");
      if (rc) return rc;
    }
    hipLaunchKernelGGL(surf3d_finish_kernel, dim3(2), dim3(256), 0, st, state, partial, counts + (int64_t)c * 2 * (1 + T), values + (int64_t)c * 6, (int)Z, T,
                       q_num, q_den);
    rc = check_launch("surface3d_stats (finish)");
    if (rc) return rc;
  }
  return 0;
}
