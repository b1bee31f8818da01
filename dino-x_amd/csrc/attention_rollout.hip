// attention_rollout.hip -- one step of the CLS row of attention rollout (Abnar & Zuidema 2020): a weighted column sum of the
// softmax rows of ONE block, all N query rows, all heads, with nothing of size N x N ever stored.
//     w_out[b][j] = residual w_in[b][j] + (1 - residual) / heads * sum_h sum_i w_in[b][i] * softmax_j( q_i . k_j / sqrt(d) )
// read straight from the packed qkv rows [B, N, 3, heads, d] (fp32 or bf16); V is never read.  The shape of dV = P^T dO of the
// attention backward with a one-column dO.  Chained from the last block down, starting from a one-hot vector, it is the row
// e_q^T Ahat_L ... Ahat_1 of the rollout matrix, Ahat_l = residual I + (1 - residual) mean_h P_l^h.
//
// Two launches.  (1) rollout_partial: one workgroup of 256 threads per (image, head) writes part[b][h][j] = sum_i w_i P^h[i][j]
// into the workspace.  (2) rollout_fold: one thread per (image, key) adds the heads in index order and the residual term.
//
// Arithmetic (the conventions of attention_rows.hip): inputs taken exactly; scores by fp32 fma in column order, times 1/sqrt(d);
// row maximum, row sum and probabilities in fp32; p = expf(s - max) / sum.  Row maximum and row sum: each lane over its keys in
// index order, then the lanes of a wave (xor butterfly), then the waves in index order.  The column sum needs no reduction between
// threads at all: key j belongs to thread j mod 256 for every query row, which adds w_i p_ij (one fma) for i = 0, 1, ... in that
// order into a register.  No atomics, one fixed order: bit-reproducible.
//
// Geometry of (1): the query rows go by in chunks of 8.  A chunk's rows sit in LDS as fp32 (8 d floats) and are read as wave-wide
// broadcasts; a thread reads each of its key rows once per chunk (16-byte loads when the rows allow it) and keeps the 8 dot
// products in registers; the chunk's scores, then their exponentials, sit in LDS as [8][N] floats, of which a thread reads back only
// what it wrote itself.  A thread owns at most RO_NMAX / 256 = 16 keys, one accumulator register each.  A chunk whose 8 weights are
// all exactly zero is skipped (its rows contribute exactly +0, so the result does not change; a non-finite q in such a row is not
// seen): the first step of a chain, whose w is one-hot, costs one chunk, not N / 8.
//
// LDS: (8 N + 8 d) floats + 256 B: 10.9 KiB at N = 261, d = 88; 44.8 KiB at N = 1370, d = 64; 136 KiB at the limits N = 4096,
// d = 256 (of 160 KiB per CU; above 64 KiB, N >= 2049 - d, the limit is raised once per process by reserve_lds).
// Modelled traffic of (1), per workgroup: K once per non-zero chunk, ceil(N / 8) N d elements at most, from L2 after the first chunk
// (K of one head: 175 KB at N = 1370, d = 64, bf16).  N^2 d fma per (image, head) is the cost; with B heads workgroups the launch
// is far from filling 256 CUs at B = 1, which is accepted for an instrument that runs once per thousand steps.
#include "common.h"

namespace dinox {

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_ROWS = 8;
constexpr int RO_DMAX = 256;
constexpr int RO_NMAX = 4096;
constexpr int RO_SLOTS = RO_NMAX / RO_THREADS;

template <int DT, bool VEC>
__global__ __launch_bounds__(RO_THREADS) void rollout_partial_kernel(const void* __restrict__ qkv, const float* __restrict__ w_in,
                                                                     float* __restrict__ part, int N, int heads, int d, float sc) {
  using T = typename elem<DT>::type;
  extern __shared__ __attribute__((aligned(16))) float ro_smem[];
  __shared__ float redm[RO_WAVES * RO_ROWS], reds[RO_WAVES * RO_ROWS];
  float* qs = ro_smem;                                                                    // [8][d] query rows of the chunk
  float* ss = ro_smem + RO_ROWS * d;                                                      // [8][N] scores, then exponentials
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = (int64_t)3 * heads * d;                                             // elements per token
  const T* base = (const T*)qkv + (int64_t)b * N * row + (int64_t)h * d;                  // q of token 0; its k is heads d further
  const float* wb = w_in + (int64_t)b * N;

  float acc[RO_SLOTS];
#pragma unroll
  for (int s = 0; s < RO_SLOTS; ++s) acc[s] = 0.f;

  for (int i0 = 0; i0 < N; i0 += RO_ROWS) {
    const int R = min(RO_ROWS, N - i0);
    float wr[RO_ROWS];
    bool any = false;
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) {
      wr[r] = r < R ? wb[i0 + r] : 0.f;
      any = any || wr[r] != 0.f;                                                          // NaN counts as non-zero
    }
    if (!any) continue;                                                                   // the same for every thread: no barrier is split

    __syncthreads();                                                                      // the previous chunk's reads of qs are over
    for (int t = tid; t < R * d; t += RO_THREADS) {
      const int r = t / d, c = t - r * d;
      qs[t] = elem<DT>::ld(base, (int64_t)(i0 + r) * row + c);
    }
    __syncthreads();

    float mx[RO_ROWS];
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) mx[r] = -INFINITY;
    for (int j = tid; j < N; j += RO_THREADS) {
      const T* kr = base + (int64_t)j * row + (int64_t)heads * d;
      float dot[RO_ROWS];
#pragma unroll
      for (int r = 0; r < RO_ROWS; ++r) dot[r] = 0.f;
      if constexpr (VEC) {
        constexpr int W = 16 / (int)sizeof(T);                                            // elements per 16-byte load: 4 fp32, 8 bf16
        for (int c = 0; c < d; c += W) {
          float kv[W];
          if constexpr (DT == DINOX_BF16) {
            const dx_u32x4 u = *reinterpret_cast<const dx_u32x4*>(kr + c);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              kv[2 * w] = __uint_as_float(u[w] << 16);
              kv[2 * w + 1] = __uint_as_float(u[w] & 0xffff0000u);
            }
          } else {
            const f32x4 u = *reinterpret_cast<const f32x4*>(kr + c);
#pragma unroll
            for (int w = 0; w < 4; ++w) kv[w] = u[w];
          }
#pragma unroll
          for (int r = 0; r < RO_ROWS; ++r) {
            if (r < R) {
              const float* qq = qs + r * d + c;
#pragma unroll
              for (int w4 = 0; w4 < W; w4 += 4) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(qq + w4);
#pragma unroll
                for (int w = 0; w < 4; ++w) dot[r] = fmaf(qv[w], kv[w4 + w], dot[r]);
              }
            }
          }
        }
      } else {
        for (int c = 0; c < d; ++c) {
          const float kv = elem<DT>::ld(kr, c);
#pragma unroll
          for (int r = 0; r < RO_ROWS; ++r)
            if (r < R) dot[r] = fmaf(qs[r * d + c], kv, dot[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < RO_ROWS; ++r) {
        if (r < R) {
          const float s = dot[r] * sc;
          ss[r * N + j] = s;
          mx[r] = fmaxf(mx[r], s);
        }
      }
    }

    // row maxima: lanes, then waves in index order (R is the same for every thread: every thread takes the barriers)
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) {
      const float m = wave_max(mx[r]);
      if (lane == 0) redm[wave * RO_ROWS + r] = m;
    }
    __syncthreads();
    float sum[RO_ROWS];
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) {
      float m = redm[r];
#pragma unroll
      for (int w = 1; w < RO_WAVES; ++w) m = fmaxf(m, redm[w * RO_ROWS + r]);
      float a = 0.f;
      if (r < R) {
        float* srow = ss + r * N;
        for (int j = tid; j < N; j += RO_THREADS) {
          const float e = expf(srow[j] - m);
          srow[j] = e;
          a += e;
        }
      }
      a = wave_sum(a);
      if (lane == 0) reds[wave * RO_ROWS + r] = a;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RO_ROWS; ++r) {
      float l = 0.f;
#pragma unroll
      for (int w = 0; w < RO_WAVES; ++w) l += reds[w * RO_ROWS + r];
      sum[r] = l;
    }

    // the column sum: thread-private, rows in index order
#pragma unroll
    for (int s = 0; s < RO_SLOTS; ++s) {
      const int j = tid + s * RO_THREADS;
      if (j < N) {
#pragma unroll
        for (int r = 0; r < RO_ROWS; ++r)
          if (r < R) acc[s] = fmaf(wr[r], ss[r * N + j] / sum[r], acc[s]);
      }
    }
  }

  float* out = part + (int64_t)bh * N;
#pragma unroll
  for (int s = 0; s < RO_SLOTS; ++s) {
    const int j = tid + s * RO_THREADS;
    if (j < N) out[j] = acc[s];
  }
}

// w_out = residual w_in + coef (part[b][0] + part[b][1] + ...), heads in index order; one thread per (image, key).
__global__ __launch_bounds__(RO_THREADS) void rollout_fold_kernel(const float* __restrict__ part, const float* __restrict__ w_in,
                                                                  float* __restrict__ w_out, int64_t total, int N, int heads, float residual,
                                                                  float coef) {
  const int64_t t = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x;
  if (t >= total) return;
  const int64_t b = t / N, j = t - b * N;
  const float* p = part + b * heads * N + j;
  float a = p[0];
  for (int h = 1; h < heads; ++h) a += p[(int64_t)h * N];
  w_out[t] = fmaf(coef, a, residual * w_in[t]);
}

static bool attention_rollout_step_ok(int B, int N, int heads, int d) {
  return B >= 1 && N >= 1 && N <= RO_NMAX && heads >= 1 && d >= 1 && d <= RO_DMAX && (int64_t)B * heads <= 0x7fffffff &&
         ceil_div((int64_t)B * N, RO_THREADS) <= 0x7fffffff;
}

}  // namespace dinox

using namespace dinox;

extern "C" int dinox_attention_rollout_step_ok(int B, int N, int heads, int d) { return attention_rollout_step_ok(B, N, heads, d) ? 1 : 0; }

extern "C" size_t dinox_attention_rollout_step_ws_bytes(int B, int N, int heads) {
  if (B < 1 || N < 1 || heads < 1 || !attention_rollout_step_ok(B, N, heads, 1)) return 0;   // what dinox_attention_rollout_step refuses (N > 4096)
  return (size_t)B * (size_t)heads * (size_t)N * sizeof(float);
}

extern "C" int dinox_attention_rollout_step(const void* qkv, const float* w_in, float* w_out, void* ws, int B, int N, int heads, int d,
                                            float residual, int dtype, void* stream) {
  DX_REQUIRE(qkv && w_in && w_out && ws, DINOX_EINVAL, "attention_rollout_step: null pointer");
  DX_REQUIRE(dtype == DINOX_F32 || dtype == DINOX_BF16, DINOX_EINVAL, "attention_rollout_step: dtype %d", dtype);
  DX_REQUIRE(attention_rollout_step_ok(B, N, heads, d), DINOX_EINVAL,
             "attention_rollout_step: B=%d N=%d heads=%d d=%d (B, heads >= 1; 1 <= N <= 4096; 1 <= d <= 256)", B, N, heads, d);
  DX_REQUIRE(residual >= 0.f && residual <= 1.f, DINOX_EINVAL, "attention_rollout_step: residual %g outside [0, 1]", (double)residual);
  const float* in_end = w_in + (size_t)B * N;
  const float* out_end = w_out + (size_t)B * N;
  DX_REQUIRE(in_end <= w_out || out_end <= w_in, DINOX_EINVAL, "attention_rollout_step: w_out must not alias w_in (the fold reads w_in)");
  hipStream_t st = as_stream(stream);
  const float sc = 1.0f / sqrtf((float)d);
  const size_t lds = (size_t)RO_ROWS * ((size_t)N + (size_t)d) * sizeof(float);
  const dim3 grid((unsigned)(B * heads)), block(RO_THREADS);
  // 16-byte key loads: every key row starts at qkv + (token 3 heads + heads + h) d elements, so d % (16 / element size) == 0 and an
  // aligned base make every row and every step inside it aligned; the LDS query rows are then 16-byte aligned too (d % 4 == 0).
  const bool vec = ((uintptr_t)qkv & 15) == 0 && d % (dtype == DINOX_BF16 ? 8 : 4) == 0;
  float* part = (float*)ws;
#define RO_LAUNCH(DT, V)                                                                                                      \
  do {                                                                                                                        \
    if (int rc = reserve_lds(reinterpret_cast<const void*>(rollout_partial_kernel<DT, V>), lds, "attention_rollout_step")) return rc; \
    hipLaunchKernelGGL((rollout_partial_kernel<DT, V>), grid, block, lds, st, qkv, w_in, part, N, heads, d, sc);               \
  } while (0)
  if (dtype == DINOX_BF16) {
    if (vec) RO_LAUNCH(DINOX_BF16, true);
    else RO_LAUNCH(DINOX_BF16, false);
  } else {
    if (vec) RO_LAUNCH(DINOX_F32, true);
    else RO_LAUNCH(DINOX_F32, false);
  }
#undef RO_LAUNCH
  if (int rc = check_launch("attention_rollout_step (partial)")) return rc;
  const int64_t total = (int64_t)B * N;
  hipLaunchKernelGGL(rollout_fold_kernel, dim3((unsigned)ceil_div(total, RO_THREADS)), block, 0, st, (const float*)part, w_in, w_out, total, N,
                     heads, residual, (1.0f - residual) / (float)heads);
  return check_launch("attention_rollout_step (fold)");
}
