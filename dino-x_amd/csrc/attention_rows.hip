// attention_rows.hip -- softmax rows of a FEW query tokens (CLS, the registers) over all keys, per head: the attention map.
// The attention cores (attention_bf16.hip, attention_flash.hip, the fp32 product form) never keep P; the reference cannot show it
// either (its fused SDPA returns no probabilities, scripts/phase5_monitor.py:make_attention_heatmap draws a patch-norm proxy).
//     probs[b][h][r][j] = softmax_j( q_{i_r} . k_j / sqrt(d) ),  i_r = query_idx[r],   lse[b][h][r] = log sum_j exp(score)
// read straight from the packed qkv rows [B, N, 3, heads, d] (fp32 or bf16).  No N x N buffer; V is never read.
//
// Arithmetic: inputs taken exactly (a bf16 product is exact in fp32); scores by fp32 fma in column order, times 1/sqrt(d); running
// maximum, sum and probabilities in fp32 (never rounded to bf16); p = expf(s - max) / sum.  Row maximum and row sum: each lane over
// its keys in index order, then the lanes of a wave (xor butterfly), then the waves in index order -- no atomics, bit-reproducible.
// A query index outside [0, N) (the C caller's error: the indices are device memory, the host cannot see them) reads nothing and
// turns its row and its lse into NaN.
//
// Geometry: one workgroup of 256 threads per (image, head); key j belongs to thread j mod 256, which reads the whole key row
// (16-byte loads when the rows allow it) and keeps the Q <= 8 dot products in registers; the query rows sit in LDS as fp32 (Q d
// floats, at most 8 KiB) and are read as wave-wide broadcasts, so K is read once.  Three sweeps over the keys of a thread: scores
// (stored in the output row, which doubles as the score buffer), sum of exponentials, probabilities.  A thread reads back only what
// it wrote itself, so no fence or inter-thread visibility is involved.
//
// Modelled bytes: K once, B N heads d elements (ViT-S/16 at 224, B = 32, bf16: 4.9 MB; ViT-L/14 at 518, B = 1: 2.8 MB), plus the
// output B heads Q N floats once to memory (its two re-reads and one overwrite stay in L2: at most Q N 4 = 44 KB per workgroup at
// 1374 tokens).  Memory-bound on K; with B heads workgroups (192 at ViT-S, 6..16 for a single image) the launch is far from
// filling 256 CUs, which is accepted for an instrument that runs once per thousand steps.
#include "common.h"

namespace dinox {

constexpr int AR_THREADS = 256;
constexpr int AR_QMAX = 8;
constexpr int AR_DMAX = 256;

template <int DT, bool VEC>
__global__ __launch_bounds__(AR_THREADS) void attention_rows_kernel(const void* __restrict__ qkv, const int* __restrict__ query_idx,
                                                                    float* probs, float* __restrict__ lse, int N, int heads, int d, int Q,
                                                                    float sc) {
  using T = typename elem<DT>::type;
  __shared__ __attribute__((aligned(16))) float qs[AR_QMAX * AR_DMAX];
  __shared__ float red[16];
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int64_t row = (int64_t)3 * heads * d;                                             // elements per token
  const T* base = (const T*)qkv + (int64_t)b * N * row + (int64_t)h * d;                  // q of token 0; its k is heads d further
  for (int t = threadIdx.x; t < Q * d; t += AR_THREADS) {
    const int r = t / d, c = t - r * d, i = query_idx[r];
    qs[t] = (i >= 0 && i < N) ? elem<DT>::ld(base, (int64_t)i * row + c) : __builtin_nanf("");
  }
  __syncthreads();

  float* out = probs + (int64_t)bh * Q * N;
  float mx[AR_QMAX];
#pragma unroll
  for (int r = 0; r < AR_QMAX; ++r) mx[r] = -INFINITY;
  for (int j = threadIdx.x; j < N; j += AR_THREADS) {
    const T* kr = base + (int64_t)j * row + (int64_t)heads * d;
    float acc[AR_QMAX];
#pragma unroll
    for (int r = 0; r < AR_QMAX; ++r) acc[r] = 0.f;
    if constexpr (VEC) {
      constexpr int W = 16 / (int)sizeof(T);                                              // elements per 16-byte load: 4 fp32, 8 bf16
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
        for (int r = 0; r < AR_QMAX; ++r) {
          if (r < Q) {
            const float* qq = qs + r * d + c;
#pragma unroll
            for (int w4 = 0; w4 < W; w4 += 4) {
              const f32x4 qv = *reinterpret_cast<const f32x4*>(qq + w4);
#pragma unroll
              for (int w = 0; w < 4; ++w) acc[r] = fmaf(qv[w], kv[w4 + w], acc[r]);
            }
          }
        }
      }
    } else {
      for (int c = 0; c < d; ++c) {
        const float kv = elem<DT>::ld(kr, c);
#pragma unroll
        for (int r = 0; r < AR_QMAX; ++r)
          if (r < Q) acc[r] = fmaf(qs[r * d + c], kv, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < AR_QMAX; ++r) {
      if (r < Q) {
        const float s = acc[r] * sc;
        out[(int64_t)r * N + j] = s;
        mx[r] = fmaxf(mx[r], s);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < AR_QMAX; ++r) {
    if (r < Q) {                                                                          // Q is uniform: every thread takes the barriers
      const float m = block_max(mx[r], red);
      float* orow = out + (int64_t)r * N;
      float a = 0.f;
      for (int j = threadIdx.x; j < N; j += AR_THREADS) a += expf(orow[j] - m);
      const float l = block_sum(a, red);
      for (int j = threadIdx.x; j < N; j += AR_THREADS) orow[j] = expf(orow[j] - m) / l;
      if (lse && threadIdx.x == 0) lse[(int64_t)bh * Q + r] = m + logf(l);
    }
  }
}

static bool attention_rows_ok(int B, int N, int heads, int d, int Q) {
  return B >= 1 && N >= 1 && heads >= 1 && d >= 1 && d <= AR_DMAX && Q >= 1 && Q <= AR_QMAX && (int64_t)B * heads <= 0x7fffffff;
}

}  // namespace dinox

using namespace dinox;

extern "C" int dinox_attention_rows_ok(int B, int N, int heads, int d, int Q) { return attention_rows_ok(B, N, heads, d, Q) ? 1 : 0; }

extern "C" int dinox_attention_rows(const void* qkv, const int* query_idx, float* probs, float* lse, int B, int N, int heads, int d, int Q,
                                    int dtype, void* stream) {
  DX_REQUIRE(qkv && query_idx && probs, DINOX_EINVAL, "attention_rows: null pointer");
  DX_REQUIRE(dtype == DINOX_F32 || dtype == DINOX_BF16, DINOX_EINVAL, "attention_rows: dtype %d", dtype);
  DX_REQUIRE(attention_rows_ok(B, N, heads, d, Q), DINOX_EINVAL,
             "attention_rows: B=%d N=%d heads=%d d=%d Q=%d (B, N, heads >= 1; 1 <= d <= 256; 1 <= Q <= 8)", B, N, heads, d, Q);
  hipStream_t st = as_stream(stream);
  const float sc = 1.0f / sqrtf((float)d);
  const dim3 grid((unsigned)(B * heads)), block(AR_THREADS);
  // 16-byte key loads: every key row starts at qkv + (token 3 heads + heads + h) d elements, so d % (16 / element size) == 0 and an
  // aligned base make every row and every step inside it aligned; the LDS query rows are then 16-byte aligned too (d % 4 == 0).
  const bool vec = ((uintptr_t)qkv & 15) == 0 && d % (dtype == DINOX_BF16 ? 8 : 4) == 0;
#define AR_LAUNCH(DT, V) hipLaunchKernelGGL((attention_rows_kernel<DT, V>), grid, block, 0, st, qkv, query_idx, probs, lse, N, heads, d, Q, sc)
  if (dtype == DINOX_BF16) {
    if (vec) AR_LAUNCH(DINOX_BF16, true);
    else AR_LAUNCH(DINOX_BF16, false);
  } else {
    if (vec) AR_LAUNCH(DINOX_F32, true);
    else AR_LAUNCH(DINOX_F32, false);
  }
#undef AR_LAUNCH
  return check_launch("attention_rows");
}
