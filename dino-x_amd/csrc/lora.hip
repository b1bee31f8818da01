// lora.hip -- the low-rank side of a LoRA-wrapped linear layer (contract: include/dinox.h).
//   y = x W^T + b + s (xl A^T) B^T: the base product is dinox_gemm; these kernels form the fp32 addend it takes as RESIDUAL, the
//   matching dX addend, and dA / dB.  A, B, u = xl A^T and v = dy B are fp32 and every sum is an fp32 fma chain in a fixed order.
// The contractions over the long axes (u = xl A^T and v = dy B over K / N columns, dA = v^T xl and dB = dy^T u over the rows) run on the
// exact-fp32 matrix instruction the project uses elsewhere (v_mfma_f32_32x32x2_f32, csrc/gemm_f32.hip): bf16 activations widen to fp32 on
// load, which is exact, so nothing on the adapter path is rounded to bf16 in either mode; per output element the instruction is one
// fp32 fma chain in the order its operands are fed.  Activation tiles go through LDS: the global reads are row-contiguous, the operand
// reads bank-contiguous.
#include <type_traits>

#include "small_common.h"

namespace dinox {

constexpr int LORA_MAX_RANK = 64;          // two 32-wide accumulator blocks per wave; u and v of one row chunk (2 x 128 x r floats) sit in LDS beside a 66 KiB tile
constexpr int LORA_GRAD_CHUNK = 128;       // rows per partial sum of dinox_lora_grad: ws holds ceil(M / 128) x (r K + N r) floats

// The vector forms read 4 elements of an activation row at once: 8 bytes of bf16, 16 of fp32.
static bool row_aligned(const void* p, int dtype) { return (reinterpret_cast<uintptr_t>(p) & (dtype == DINOX_BF16 ? 7 : 15)) == 0; }

// ---------------------------------------------------------------- the shared tile machinery: 128 rows x 128 columns of an activation in LDS
// A workgroup is 256 threads = 4 waves; a lane is (c = lane & 31, h = lane >> 5).  v_mfma_f32_32x32x2_f32: the first operand of lane
// (c, h) is element (row c, k h), the second (k h, column c); accumulator e of lane (c, h) is output (row (e & 3) + 8 (e >> 2) + 4 h,
// column c).  Four consecutive instructions take k = 8 g + 4 h + s, s = 0 .. 3, so a lane's four values are one aligned 16-byte read.
constexpr int LT_ROWS = LORA_GRAD_CHUNK;   // 128
constexpr int LT_COLS = 128;
constexpr int LT_PITCH = 132;              // floats: 16-byte aligned rows; 32 rows at this pitch spread over all banks for the 16-byte reads
constexpr int LT_FLOATS = LT_ROWS * LT_PITCH;

__device__ __forceinline__ int mfma_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

// Xs[m][q] = X[row0 + m][c0 + q] as fp32 for m < 128, q < 128; zero past `rows` and past column C.  32 threads per row: contiguous reads.
template <int DT>
__device__ __forceinline__ void stage_tile(const void* __restrict__ X, int64_t row0, int rows, int C, int c0, bool vec, float* Xs, int tid) {
  const int q = tid & 31, rr = tid >> 5, col = c0 + 4 * q;
#pragma unroll 4
  for (int p = 0; p < LT_ROWS / 8; ++p) {
    const int m = p * 8 + rr;
    fvec<4> v = vzero<4>();
    if (m < rows && col < C) {
      const int64_t o = (row0 + m) * (int64_t)C + col;
      if (vec) {                                    // C % 4 == 0: col < C means col + 4 <= C
        v = ld_dt<DT, 4>(X, o);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (col + i < C) v.e[i] = elem<DT>::ld(X, o + i);
      }
    }
    *reinterpret_cast<f32x4*>(Xs + m * LT_PITCH + 4 * q) = f32x4{v.e[0], v.e[1], v.e[2], v.e[3]};
  }
}

// acc[jb] (row i of this wave's 32 rows, column j = 32 jb + c) += sum over the staged columns of Xs[32 w + i][q] S(j, c0 + q).
// LAYOUT 0: S(j, col) = S[j * C + col]; LAYOUT 1: S(j, col) = S[col * r + j].  svec (LAYOUT 0): C % 4 == 0 and S 16-byte aligned.
template <int LAYOUT>
__device__ __forceinline__ void dot_tile(const float* Xs, const float* __restrict__ S, int C, int c0, int r, bool svec, int w, int c, int h,
                                         f32x16 (&acc)[2]) {
  const int njb = (r + 31) >> 5;
  for (int g = 0; g < LT_COLS / 8; ++g) {
    if (c0 + 8 * g >= C) break;                     // the rest of the tile is past the last column (zeros in Xs)
    const int kq = 8 * g + 4 * h, col = c0 + kq;
    const f32x4 a = *reinterpret_cast<const f32x4*>(Xs + (32 * w + c) * LT_PITCH + kq);
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      if (jb >= njb) break;
      const int j = 32 * jb + c;
      fvec<4> b = vzero<4>();
      if (j < r && col < C) {
        if constexpr (LAYOUT == 0) {
          if (svec) {
            b = ld_f32<4>(S + (int64_t)j * C + col);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (col + i < C) b.e[i] = S[(int64_t)j * C + col + i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (col + i < C) b.e[i] = S[(int64_t)(col + i) * r + j];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b.e[i], acc[jb], 0, 0, 0);
    }
  }
}

// out[m][j] = sum_col X[row0 + m][col] S(j, col) for the 128 rows of a chunk (rows past `rows` come out as 0), all j < r.  `out` is the
// chunk's [128][r] block in LDS or global memory; only rows < store_rows are written.
template <int DT, int LAYOUT>
__device__ __forceinline__ void chunk_dot(const void* __restrict__ X, int64_t row0, int rows, int C, const float* __restrict__ S, int r, bool vec,
                                          bool svec, float* Xs, float* out, int store_rows, int tid) {
  const int lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
  f32x16 acc[2];
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[jb][e] = 0.f;
  for (int c0 = 0; c0 < C; c0 += LT_COLS) {
    stage_tile<DT>(X, row0, rows, C, c0, vec, Xs, tid);
    __syncthreads();
    dot_tile<LAYOUT>(Xs, S, C, c0, r, svec, w, c, h, acc);
    __syncthreads();                                // the next tile overwrites Xs
  }
#pragma unroll
  for (int jb = 0; jb < 2; ++jb) {
    const int j = 32 * jb + c;
    if (j >= r) continue;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = 32 * w + mfma_row(e, h);
      if (m < store_rows) out[m * r + j] = acc[jb][e];
    }
  }
}

// ---------------------------------------------------------------- down: u[M][r] = x . S, a 128-row chunk per workgroup
template <int DT, int LAYOUT>
__global__ __launch_bounds__(256) void lora_down_kernel(const void* __restrict__ x, const float* __restrict__ S, float* __restrict__ u, int64_t M,
                                                        int Kd, int r, int vec, int svec) {
  extern __shared__ __attribute__((aligned(16))) float lora_lds[];
  const int64_t row0 = (int64_t)blockIdx.x * LT_ROWS;
  const int rows = (int)(M - row0 < LT_ROWS ? M - row0 : LT_ROWS);
  chunk_dot<DT, LAYOUT>(x, row0, rows, Kd, S, r, vec != 0, svec != 0, lora_lds, u + row0 * r, rows, threadIdx.x);
}

// ---------------------------------------------------------------- up: t[M][N] = s u . S (+ res)
// A thread owns 4 rows x VEC columns; the r-long chains run in ascending j.  LAYOUT 0: S(n, j) = S[n * r + j]; LAYOUT 1: S(n, j) = S[j * N + n].
template <int LAYOUT, int VEC>
__global__ __launch_bounds__(256) void lora_up_kernel(const float* __restrict__ u, const float* __restrict__ S, const float* res, float* t, float s,
                                                      int64_t M, int N, int r, int r4) {
  const int64_t ncg = N / VEC;                       // VEC == 4 only when N % 4 == 0
  const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (id >= ceil_div(M, 4) * ncg) return;
  const int64_t m0 = (id / ncg) * 4;
  const int n0 = (int)(id % ncg) * VEC;
  const float* urow[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) urow[m] = u + (m0 + m < M ? m0 + m : M - 1) * r;
  float acc[4][VEC];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[m][i] = 0.f;
  // r4 (LAYOUT 0, VEC 4): r % 4 == 0 and u, S 16-byte aligned -- four j at a time from aligned float4 of the rows of S and u; every
  // chain still runs in ascending j
  for (int j = 0; LAYOUT == 0 && VEC == 4 && r4 && j < r; j += 4) {
    float4 sq[VEC], uq[4];
#pragma unroll
    for (int i = 0; i < VEC; ++i) sq[i] = *reinterpret_cast<const float4*>(S + (int64_t)(n0 + i) * r + j);
#pragma unroll
    for (int m = 0; m < 4; ++m) uq[m] = *reinterpret_cast<const float4*>(urow[m] + j);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        float a = acc[m][i];
        a = fmaf(uq[m].x, sq[i].x, a);
        a = fmaf(uq[m].y, sq[i].y, a);
        a = fmaf(uq[m].z, sq[i].z, a);
        acc[m][i] = fmaf(uq[m].w, sq[i].w, a);
      }
  }
  for (int j = (LAYOUT == 0 && VEC == 4 && r4) ? r : 0; j < r; ++j) {
    float sv[VEC];
    if constexpr (LAYOUT == 1 && VEC == 4) {
      const float4 q = *reinterpret_cast<const float4*>(S + (int64_t)j * N + n0);
      sv[0] = q.x, sv[1] = q.y, sv[2] = q.z, sv[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < VEC; ++i) sv[i] = LAYOUT == 0 ? S[(int64_t)(n0 + i) * r + j] : S[(int64_t)j * N + n0 + i];
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float um = urow[m][j];
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc[m][i] = fmaf(um, sv[i], acc[m][i]);
    }
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (m0 + m >= M) break;
    const int64_t o = (m0 + m) * N + n0;
    if constexpr (VEC == 4) {
      float4 q = make_float4(s * acc[m][0], s * acc[m][1], s * acc[m][2], s * acc[m][3]);
      if (res) {
        const float4 a = *reinterpret_cast<const float4*>(res + o);
        q.x += a.x, q.y += a.y, q.z += a.z, q.w += a.w;
      }
      *reinterpret_cast<float4*>(t + o) = q;
    } else {
      const float q = s * acc[m][0];
      t[o] = res ? q + res[o] : q;
    }
  }
}

// ---------------------------------------------------------------- grad: dA = s v^T xl, dB = s dy^T u
// Workgroup c: rows [128 c, 128 c + 128).  Pass 1 forms the chunk's u = xl A^T and v = dy B in LDS (chunk_dot: the down kernel's body).
// Pass 2 stages the tiles of xl (for dA, against v) and of dy (for dB, against u) once more -- from the caches pass 1 filled -- and
// contracts over the chunk's rows: wave w owns 32 of a tile's 128 columns, the row order is the instruction order, nothing is summed
// across waves.  Partials: ws[c][r K + N r], unscaled.
// P(j, col) = sum_m T[m][j] Xs[m][32 w + c] for j in [32 jb, 32 jb + 32): T is u or v in LDS ([128][r]).
__device__ __forceinline__ f32x16 outer_tile(const float* Xs, const float* Ts, int r, int w, int c, int h, int jb) {
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int j = 32 * jb + c;
  const bool in = j < r;
#pragma unroll 4
  for (int g = 0; g < LT_ROWS / 8; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 8 * g + 4 * h + i;
      const float a = in ? Ts[m * r + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, Xs[m * LT_PITCH + 32 * w + c], acc, 0, 0, 0);
    }
  return acc;
}

template <int DT>
__global__ __launch_bounds__(256) void lora_grad_partial_kernel(const void* __restrict__ xl, const void* __restrict__ dy, const float* __restrict__ A,
                                                                const float* __restrict__ B, float* __restrict__ ws, int64_t M, int K, int N, int r,
                                                                int vecK, int vecN, int avec) {
  extern __shared__ __attribute__((aligned(16))) float lora_lds[];
  float* Xs = lora_lds;                              // [128][132]
  float* u_s = lora_lds + LT_FLOATS;                 // [128][r]
  float* v_s = u_s + LT_ROWS * r;                    // [128][r]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 31, h = lane >> 5;
  const int64_t row0 = (int64_t)blockIdx.x * LT_ROWS;
  const int rows = (int)(M - row0 < LT_ROWS ? M - row0 : LT_ROWS);
  // all 128 rows of u and v are written: rows past the chunk's end are exact zeros (their Xs rows are)
  chunk_dot<DT, 0>(xl, row0, rows, K, A, r, vecK != 0, avec != 0, Xs, u_s, LT_ROWS, tid);
  chunk_dot<DT, 1>(dy, row0, rows, N, B, r, vecN != 0, false, Xs, v_s, LT_ROWS, tid);
  __syncthreads();
  const int njb = (r + 31) >> 5;
  const int64_t nA = (int64_t)r * K;
  float* wsc = ws + (int64_t)blockIdx.x * (nA + (int64_t)N * r);
  for (int c0 = 0; c0 < K; c0 += LT_COLS) {
    stage_tile<DT>(xl, row0, rows, K, c0, vecK != 0, Xs, tid);
    __syncthreads();
    const int col = c0 + 32 * w + c;
    if (c0 + 32 * w < K)                             // wave-uniform
      for (int jb = 0; jb < njb; ++jb) {
        const f32x16 acc = outer_tile(Xs, v_s, r, w, c, h, jb);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = 32 * jb + mfma_row(e, h);
          if (j < r && col < K) wsc[(int64_t)j * K + col] = acc[e];
        }
      }
    __syncthreads();
  }
  for (int c0 = 0; c0 < N; c0 += LT_COLS) {
    stage_tile<DT>(dy, row0, rows, N, c0, vecN != 0, Xs, tid);
    __syncthreads();
    const int col = c0 + 32 * w + c;
    if (c0 + 32 * w < N)
      for (int jb = 0; jb < njb; ++jb) {
        const f32x16 acc = outer_tile(Xs, u_s, r, w, c, h, jb);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int j = 32 * jb + mfma_row(e, h);
          if (j < r && col < N) wsc[nA + (int64_t)col * r + j] = acc[e];
        }
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void lora_grad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dA, float* __restrict__ dB, float s,
                                                               int nchunks, int64_t nA, int64_t nB) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x, n = nA + nB;
  if (e >= n) return;
  float acc = 0.f;
#pragma unroll 8
  for (int c = 0; c < nchunks; ++c) acc += ws[(int64_t)c * n + e];
  if (e < nA) dA[e] = s * acc;
  else dB[e - nA] = s * acc;
}

// ---------------------------------------------------------------- dropout without a stored mask
__host__ __device__ static inline uint32_t lora_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x21f0aaadu;
  x ^= x >> 15;
  x *= 0x735a2d97u;
  x ^= x >> 15;
  return x;
}
__device__ __forceinline__ bool lora_keep(uint64_t i, uint32_t key, uint32_t thr) {
  return (lora_mix((uint32_t)i ^ lora_mix((uint32_t)(i >> 32) + key)) >> 8) >= thr;
}

template <int DT>
__global__ __launch_bounds__(256) void lora_dropout_kernel(const void* in, void* out, int64_t n, float scale, uint32_t key, uint32_t thr, int vec) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= n) return;
  if (vec && i0 + 4 <= n) {
    fvec<4> v = ld_dt<DT, 4>(in, i0);
#pragma unroll
    for (int i = 0; i < 4; ++i) v.e[i] = lora_keep((uint64_t)(i0 + i), key, thr) ? v.e[i] * scale : 0.f;
    st_dt<DT, 4>(out, i0, v);
  } else {
    for (int64_t i = i0; i < n && i < i0 + 4; ++i)
      elem<DT>::st(out, i, lora_keep((uint64_t)i, key, thr) ? elem<DT>::ld(in, i) * scale : 0.f);
  }
}

static uint32_t lora_dropout_key(uint64_t seed, uint64_t offset) {
  const uint32_t ks = lora_mix((uint32_t)seed ^ lora_mix((uint32_t)(seed >> 32) + 0x9e3779b9u));
  return lora_mix((uint32_t)offset ^ lora_mix((uint32_t)(offset >> 32) + ks));
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
static bool lora_rank_ok(int r) { return r >= 1 && r <= LORA_MAX_RANK; }
static bool lora_dim_ok(int d) { return d >= 1 && d <= (1 << 20); }
static bool lora_rows_ok(int64_t M) { return M >= 1 && M <= 0x7fffffff; }
static bool lora_up_grid_ok(int64_t M, int N) { return ceil_div(ceil_div(M, 4) * (int64_t)N, 256) <= 0x7fffffff; }

extern "C" int dinox_lora_down(const void* x, const float* small, float* u, int64_t M, int K, int r, int small_layout, int dtype, void* stream) {
  DX_REQUIRE(x && small && u, DINOX_EINVAL, "lora_down: null pointer");
  DX_REQUIRE(dtype_ok(dtype) && (small_layout == 0 || small_layout == 1), DINOX_EINVAL, "lora_down: dtype %d, small_layout %d", dtype,
             small_layout);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_down: r=%d (1 <= r <= %d)", r, LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(K), DINOX_EINVAL, "lora_down: M=%lld K=%d (1 <= M <= 2^31 - 1; 1 <= K <= 2^20)", (long long)M, K);
  hipStream_t st = as_stream(stream);
  const int vec = K % 4 == 0 && row_aligned(x, dtype), svec = small_layout == 0 && K % 4 == 0 && aligned16(small);
  const unsigned grid = (unsigned)ceil_div(M, (int64_t)LT_ROWS);
  const size_t lds = (size_t)LT_FLOATS * sizeof(float);
  auto go = [&](auto dt, auto lay) -> int {
    auto kern = lora_down_kernel<decltype(dt)::value, decltype(lay)::value>;
    const int rc = reserve_lds((const void*)kern, lds, "lora_down");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, x, small, u, M, K, r, vec, svec);
    return 0;
  };
  auto by_lay = [&](auto dt) { return small_layout ? go(dt, std::integral_constant<int, 1>{}) : go(dt, std::integral_constant<int, 0>{}); };
  const int rc = dtype == DINOX_BF16 ? by_lay(std::integral_constant<int, DINOX_BF16>{}) : by_lay(std::integral_constant<int, DINOX_F32>{});
  return rc ? rc : check_launch("lora_down");
}

// The up product t = s u . S (+ res), for dinox_lora_up and, with B as the rows and A stored [r][K], dinox_lora_merge.
static int lora_up(const float* u, const float* S, const float* res, float* t, float s, int64_t M, int N, int r, int layout, hipStream_t st) {
  const bool vec = N % 4 == 0 && aligned16(t, res) && (layout == 0 || aligned16(S));
  const int64_t items = ceil_div(M, 4) * (int64_t)(vec ? N / 4 : N);
  const unsigned grid = (unsigned)ceil_div(items, 256);
  const int r4 = layout == 0 && r % 4 == 0 && aligned16(S, u);
  auto go = [&](auto lay, auto v) {
    hipLaunchKernelGGL((lora_up_kernel<decltype(lay)::value, decltype(v)::value>), dim3(grid), dim3(256), 0, st, u, S, res, t, s, M, N, r, r4);
  };
  auto by_vec = [&](auto lay) { vec ? go(lay, std::integral_constant<int, 4>{}) : go(lay, std::integral_constant<int, 1>{}); };
  layout ? by_vec(std::integral_constant<int, 1>{}) : by_vec(std::integral_constant<int, 0>{});
  return check_launch("lora_up");
}

extern "C" int dinox_lora_up(const float* u, const float* small, const float* res, float* t, float s, int64_t M, int N, int r, int small_layout,
                             void* stream) {
  DX_REQUIRE(u && small && t, DINOX_EINVAL, "lora_up: null pointer");
  DX_REQUIRE(small_layout == 0 || small_layout == 1, DINOX_EINVAL, "lora_up: small_layout %d", small_layout);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_up: r=%d (1 <= r <= %d)", r, LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(N) && lora_up_grid_ok(M, N), DINOX_EINVAL,
             "lora_up: M=%lld N=%d (1 <= M <= 2^31 - 1; 1 <= N <= 2^20; M N / 4 <= 2^39)", (long long)M, N);
  return lora_up(u, small, res, t, s, M, N, r, small_layout, as_stream(stream));
}

static int64_t lora_grad_chunks(int64_t M) { return ceil_div(M, (int64_t)LORA_GRAD_CHUNK); }

extern "C" int64_t dinox_lora_grad_ws_bytes(int64_t M, int K, int N, int r) {
  if (!(lora_rows_ok(M) && lora_dim_ok(K) && lora_dim_ok(N) && lora_rank_ok(r))) return 0;
  return lora_grad_chunks(M) * ((int64_t)r * K + (int64_t)N * r) * (int64_t)sizeof(float);
}

extern "C" int dinox_lora_grad(const void* xl, const void* dy, const float* A, const float* B, float s, float* dA, float* dB, float* ws, int64_t M,
                               int K, int N, int r, int dtype, void* stream) {
  DX_REQUIRE(xl && dy && A && B && dA && dB && ws, DINOX_EINVAL, "lora_grad: null pointer");
  DX_REQUIRE(dtype_ok(dtype), DINOX_EINVAL, "lora_grad: dtype %d", dtype);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_grad: r=%d (1 <= r <= %d)", r, LORA_MAX_RANK);
  DX_REQUIRE(lora_rows_ok(M) && lora_dim_ok(K) && lora_dim_ok(N), DINOX_EINVAL, "lora_grad: M=%lld K=%d N=%d (1 <= M <= 2^31 - 1; 1 <= K, N <= 2^20)",
             (long long)M, K, N);
  hipStream_t st = as_stream(stream);
  const int vecK = K % 4 == 0 && row_aligned(xl, dtype), vecN = N % 4 == 0 && row_aligned(dy, dtype), avec = K % 4 == 0 && aligned16(A);
  const int64_t chunks = lora_grad_chunks(M), nA = (int64_t)r * K, nB = (int64_t)N * r;
  const size_t lds = ((size_t)LT_FLOATS + (size_t)2 * LT_ROWS * r) * sizeof(float);      // 66 KiB + 1 KiB per rank: 130 KiB at r = 64
  auto go = [&](auto kern) -> int {
    const int rc = reserve_lds((const void*)kern, lds, "lora_grad");
    if (rc) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)chunks), dim3(256), lds, st, xl, dy, A, B, ws, M, K, N, r, vecK, vecN, avec);
    return check_launch("lora_grad (partials)");
  };
  const int rc = dtype == DINOX_BF16 ? go(lora_grad_partial_kernel<DINOX_BF16>) : go(lora_grad_partial_kernel<DINOX_F32>);
  if (rc) return rc;
  hipLaunchKernelGGL(lora_grad_reduce_kernel, dim3((unsigned)ceil_div(nA + nB, 256)), dim3(256), 0, st, ws, dA, dB, s, (int)chunks, nA, nB);
  return check_launch("lora_grad (sum)");
}

extern "C" int dinox_lora_dropout(const void* in, void* out, int64_t n, float p, uint64_t seed, uint64_t offset, int dtype, void* stream) {
  DX_REQUIRE(in && out, DINOX_EINVAL, "lora_dropout: null pointer");
  DX_REQUIRE(dtype_ok(dtype), DINOX_EINVAL, "lora_dropout: dtype %d", dtype);
  DX_REQUIRE(p >= 0.f && p < 1.f, DINOX_EINVAL, "lora_dropout: p=%g outside [0, 1)", (double)p);
  DX_REQUIRE(n >= 1 && n <= ((int64_t)1 << 40), DINOX_EINVAL, "lora_dropout: n=%lld (1 <= n <= 2^40)", (long long)n);
  const int vec = row_aligned(in, dtype) && row_aligned(out, dtype);
  const uint32_t key = lora_dropout_key(seed, offset);
  const uint32_t thr = (uint32_t)ceil((double)p * 16777216.0);          // keep iff the 24-bit draw >= p 2^24
  const float scale = 1.0f / (1.0f - p);
  const unsigned grid = (unsigned)ceil_div(ceil_div(n, 4), 256);
  DX_LAUNCH_DT(lora_dropout_kernel, dtype, dim3(grid), dim3(256), as_stream(stream), in, out, n, scale, key, thr, vec);
  return check_launch("lora_dropout");
}

extern "C" int dinox_lora_merge(const float* w, const float* A, const float* B, float* w_out, float s, int sign, int N, int K, int r, void* stream) {
  DX_REQUIRE(w && A && B && w_out, DINOX_EINVAL, "lora_merge: null pointer");
  DX_REQUIRE(sign == 1 || sign == -1, DINOX_EINVAL, "lora_merge: sign %d (+1 merges, -1 unmerges)", sign);
  DX_REQUIRE(lora_rank_ok(r), DINOX_EINVAL, "lora_merge: r=%d (1 <= r <= %d)", r, LORA_MAX_RANK);
  DX_REQUIRE(lora_dim_ok(N) && lora_dim_ok(K) && lora_up_grid_ok(N, K), DINOX_EINVAL, "lora_merge: N=%d K=%d (1 <= N, K <= 2^20)", N, K);
  // w_out[n][k] = w[n][k] + (sign s) sum_j B[n][j] A[j][k]: the up product with B as its rows and A stored [r][K]
  return lora_up(B, A, w, w_out, (float)sign * s, N, K, r, 1, as_stream(stream));
}
