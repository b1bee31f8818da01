// gram.hip -- second moments of the columns of a tall fp32 matrix in one pass: with z_i = x_i - shift (fp32 subtraction, shift = NULL: z = x)
//   gram[a][b] = sum_i z_ia z_ib      colsum[a] = sum_i z_ia            (double [D][D] and [D])
// Feeds the host side of dinox.probes (ridge normal equations, per-dataset covariance and centroids): callers append a target column to x
// and read X^T y and y^T y from the same Gram.  Replaces the reference's host NumPy / scikit-learn passes over the embedding matrix
// (scripts/evaluate_panorgan.py:569-697).
//
// Products on the exact-fp32 MFMA (the instruction of gemm_f32.hip / retrieval.hip); the token dimension i is the MFMA's K, so x is staged
// as it lies in memory: 16 rows x 128 columns per operand and slab, no transpose.  The output is a few 128 x 128 tiles (only those on or
// above the diagonal are computed), far fewer than the chip has CUs, so the rows are split over about GRAM_TARGET_GROUPS workgroups:
//   1. gram_sweep:   grid = (upper tiles, row splits); fp32 partial tile (and, on diagonal tiles, fp32 partial column sums) to ws.
//   2. gram_finish:  one thread per output element on or above the diagonal sums its partials in ascending split order in double and
//                    writes it and its mirror image: the result is symmetric to the bit.
// Plain stores, no atomics: two runs give identical bits.  Rows past N and columns past D are staged as exact zeros (the shift is not
// applied to them), so they contribute nothing.  Non-finite inputs propagate through the sums; no address or loop depends on a value.
#include "common.h"

namespace dinox {

constexpr int GR_T = 128, GR_BK = 16, GR_THREADS = 256;
constexpr int GR_LD = GR_T + 4;                  // LDS row pitch (floats): keeps the 16-byte staging stores aligned, rows 4 banks apart
constexpr int GR_DMAX = 1024;
constexpr int64_t GRAM_TARGET_GROUPS = 512;      // about one resident round (two workgroups of 17 KB LDS and 64 accumulators per CU)

struct GramPlan {
  int T, tiles;                                  // 128-wide column panels; tiles on or above the diagonal
  int64_t splits, rows_per_split;                // rows_per_split is a multiple of GR_BK
};

// A pure function of (N, D): dinox_gram_ws_bytes and the launch agree.
static GramPlan gram_plan(int64_t N, int64_t D) {
  GramPlan p;
  p.T = (int)ceil_div(D, (int64_t)GR_T);
  p.tiles = p.T * (p.T + 1) / 2;
  const int64_t slabs = ceil_div(N, (int64_t)GR_BK);
  int64_t want = ceil_div(GRAM_TARGET_GROUPS, (int64_t)p.tiles);
  if (want > slabs) want = slabs;
  const int64_t slabs_per_split = ceil_div(slabs, want);
  p.splits = ceil_div(slabs, slabs_per_split);   // no empty split
  p.rows_per_split = slabs_per_split * GR_BK;
  return p;
}

// 16 rows x 128 columns of z: 512 quads, two per thread; 32 neighbouring threads read 512 contiguous bytes of a row.
template <bool VEC>
__device__ __forceinline__ void gram_fetch(const float* __restrict__ x, int64_t ldx, int64_t row0, int64_t row_hi, int64_t col0, int64_t D,
                                           const float (&sh)[4], f32x4 (&v)[2]) {
  const int t = threadIdx.x;
  const int64_t gc = col0 + 4 * (t & 31);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int64_t gr = row0 + (t >> 5) + 8 * i;
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    if (gr < row_hi && gc < D) {
      const float* p = x + gr * ldx + gc;
      if (VEC && gc + 4 <= D) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) z[cc] = q[cc] - sh[cc];
      } else {
#pragma unroll
        for (int cc = 0; cc < 4; ++cc)
          if (gc + cc < D) z[cc] = p[cc] - sh[cc];
      }
    }
    v[i] = z;
  }
}

__device__ __forceinline__ void gram_put(const f32x4 (&v)[2], float (*dst)[GR_LD]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&dst[(t >> 5) + 8 * i][4 * (t & 31)]) = v[i];
}

// ------------------------------------------------------------------------------------------ 1. sweep
template <bool VEC>
__global__ __launch_bounds__(GR_THREADS) void gram_sweep(const float* __restrict__ x, int64_t ldx, int64_t N, int64_t D,
                                                         const float* __restrict__ shift, int64_t rows_per_split, int T, int tiles,
                                                         float* __restrict__ ws_tile, float* __restrict__ ws_cs) {
  __shared__ __attribute__((aligned(16))) float As[GR_BK][GR_LD];
  __shared__ __attribute__((aligned(16))) float Bs[GR_BK][GR_LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;           // wr: which 64 columns of the a panel, wc: which 64 of the b panel
  int tb = blockIdx.x, ta = 0;                   // tile number -> (ta, tb), ta <= tb, rows of the upper triangle in order
  while (tb >= T - ta) {
    tb -= T - ta;
    ++ta;
  }
  tb += ta;
  const bool diag = ta == tb;
  const int64_t row_lo = (int64_t)blockIdx.y * rows_per_split;
  const int64_t row_hi = row_lo + rows_per_split < N ? row_lo + rows_per_split : N;
  const int64_t ca = (int64_t)ta * GR_T, cb = (int64_t)tb * GR_T;

  float sa[4], sb[4];
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    const int64_t ga = ca + 4 * (threadIdx.x & 31) + cc, gb = cb + 4 * (threadIdx.x & 31) + cc;
    sa[cc] = (shift && ga < D) ? shift[ga] : 0.f;
    sb[cc] = (shift && gb < D) ? shift[gb] : 0.f;
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float cs = 0.f;                                // column ca + threadIdx.x of a diagonal tile (threads 0..127)
  const float (*Bp)[GR_LD] = diag ? As : Bs;

  f32x4 va[2], vb[2];
  gram_fetch<VEC>(x, ldx, row_lo, row_hi, ca, D, sa, va);
  if (!diag) gram_fetch<VEC>(x, ldx, row_lo, row_hi, cb, D, sb, vb);
  for (int64_t r0 = row_lo; r0 < row_hi; r0 += GR_BK) {
    gram_put(va, As);
    if (!diag) gram_put(vb, Bs);
    __syncthreads();
    if (r0 + GR_BK < row_hi) {                   // next slab: in flight under the products below
      gram_fetch<VEC>(x, ldx, r0 + GR_BK, row_hi, ca, D, sa, va);
      if (!diag) gram_fetch<VEC>(x, ldx, r0 + GR_BK, row_hi, cb, D, sb, vb);
    }
#pragma unroll
    for (int kk = 0; kk < GR_BK; kk += 2) {
      const int kr = kk + h;
      const float a0 = As[kr][wr * 64 + c], a1 = As[kr][wr * 64 + 32 + c];
      const float b0 = Bp[kr][wc * 64 + c], b1 = Bp[kr][wc * 64 + 32 + c];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (diag && threadIdx.x < GR_T) {
#pragma unroll
      for (int kr = 0; kr < GR_BK; ++kr) cs += As[kr][threadIdx.x];
    }
    __syncthreads();
  }

  // acc[i][j][e] = tile element (a = wr 64 + i 32 + (e & 3) + 8 (e >> 2) + 4 h, b = wc 64 + j 32 + c)
  float* out = ws_tile + ((int64_t)blockIdx.y * tiles + blockIdx.x) * (GR_T * GR_T);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) out[(wr * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h) * GR_T + wc * 64 + j * 32 + c] = acc[i][j][e];
  if (diag && threadIdx.x < GR_T) ws_cs[((int64_t)blockIdx.y * T + ta) * GR_T + threadIdx.x] = cs;
}

// ------------------------------------------------------------------------------------------ 2. sum of the splits, mirror
__global__ __launch_bounds__(256) void gram_finish(const float* __restrict__ ws_tile, const float* __restrict__ ws_cs, int64_t D, int T,
                                                   int tiles, int64_t splits, double* __restrict__ gram, double* __restrict__ colsum) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item < D * D) {
    const int64_t a = item / D, b = item - a * D;
    if (a > b) return;                           // written by (b, a)'s mirror store
    const int ta = (int)(a >> 7), tb = (int)(b >> 7);
    const int tile = ta * T - ta * (ta - 1) / 2 + (tb - ta);
    const float* p = ws_tile + (int64_t)tile * (GR_T * GR_T) + (a & 127) * GR_T + (b & 127);
    double s = 0.0;
    for (int64_t k = 0; k < splits; ++k) s += (double)p[k * tiles * (GR_T * GR_T)];       // ascending split = ascending rows: a fixed order
    gram[a * D + b] = s;
    gram[b * D + a] = s;
  } else if (item < D * D + D) {
    const int64_t j = item - D * D;
    double s = 0.0;
    for (int64_t k = 0; k < splits; ++k) s += (double)ws_cs[k * T * GR_T + j];
    colsum[j] = s;
  }
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_gram_ws_bytes(int64_t N, int64_t D) {
  if (N < 1 || D < 1 || D > GR_DMAX) return 0;   // what dinox_gram_f32 refuses
  const GramPlan p = gram_plan(N, D);
  return p.splits * ((int64_t)p.tiles * GR_T * GR_T + (int64_t)p.T * GR_T) * 4;
}

extern "C" int dinox_gram_f32(const float* x, int64_t ldx, int64_t N, int64_t D, const float* shift, double* gram, double* colsum, void* ws,
                              void* stream) {
  DX_REQUIRE(x && gram && colsum && ws, DINOX_EINVAL, "gram_f32: null pointer");
  DX_REQUIRE(N >= 1 && D >= 1 && D <= GR_DMAX && ldx >= D, DINOX_EINVAL, "gram_f32: N=%lld D=%lld (1..%d) ldx=%lld", (long long)N, (long long)D,
             GR_DMAX, (long long)ldx);
  const GramPlan p = gram_plan(N, D);
  float* ws_tile = (float*)ws;
  float* ws_cs = ws_tile + p.splits * p.tiles * (GR_T * GR_T);
  const bool vec = (uintptr_t)x % 16 == 0 && ldx % 4 == 0;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)p.tiles, (unsigned)p.splits);
#define GRAM_SWEEP(V) \
  hipLaunchKernelGGL(gram_sweep<V>, grid, dim3(GR_THREADS), 0, st, x, ldx, N, D, shift, p.rows_per_split, p.T, p.tiles, ws_tile, ws_cs)
  if (vec) GRAM_SWEEP(true); else GRAM_SWEEP(false);
#undef GRAM_SWEEP
  if (int rc = check_launch("gram_sweep")) return rc;
  hipLaunchKernelGGL(gram_finish, dim3((unsigned)ceil_div(D * D + D, (int64_t)256)), dim3(256), 0, st, (const float*)ws_tile, (const float*)ws_cs,
                     D, p.T, p.tiles, p.splits, gram, colsum);
  return check_launch("gram_finish");
}
