// gemm.hip -- dinox_gemm dispatcher + column sums.
#include <cstring>

#include "common.h"
#include "kernels.h"

namespace dinox {

// out[n] (+)= sum_m x[m][n] in a FIXED order (no atomics: bit-reproducible).  Block = 1024 threads = 64 columns x 16 row-groups; a
// block owns 64 columns and all M rows: thread (c, g) sums rows g, g + 16, ... (four independent partial sums in flight), the 16
// groups meet in LDS as a fixed tree.  Only the fp32 parity mode and bias-only backward passes come here (the bf16 dW products
// produce their bias gradient themselves), so a grid of N / 64 workgroups is enough.
template <int DT>
__global__ __launch_bounds__(1024) void colsum_kernel(const void* __restrict__ x, float* __restrict__ out, int64_t M,
                                                      int64_t N, int64_t ldx, int accumulate) {
  __shared__ float red[16][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 64 + c;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (n < N) {
    int64_t r = g;
    for (; r + 48 < M; r += 64) {
      s0 += elem<DT>::ld(x, r * ldx + n);
      s1 += elem<DT>::ld(x, (r + 16) * ldx + n);
      s2 += elem<DT>::ld(x, (r + 32) * ldx + n);
      s3 += elem<DT>::ld(x, (r + 48) * ldx + n);
    }
    for (; r < M; r += 16) s0 += elem<DT>::ld(x, r * ldx + n);
  }
  red[g][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && n < N) {
    float t[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) t[k] = red[k][c];
    const float v = (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))) +
                    (((t[8] + t[9]) + (t[10] + t[11])) + ((t[12] + t[13]) + (t[14] + t[15])));
    out[n] = (accumulate ? out[n] : 0.f) + v;
  }
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- per-launch timing (dinox_gemm_timer_*: diagnostic, bench.py's roofline)
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>
namespace {
struct TimerRec {
  int64_t launches = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
typedef std::tuple<std::string, int64_t, int64_t, int64_t, int64_t, int, int, int, int, int> TimerKey;   // kernel M N K batch epi in out aux shared_b
std::mutex g_timer_mu;
bool g_timer_on = false;
int g_timer_every = 16;
uint64_t g_timer_n = 0;
std::map<TimerKey, TimerRec> g_timer;
std::vector<hipEvent_t> g_timer_pool;

hipEvent_t timer_event() {
  if (!g_timer_pool.empty()) {
    hipEvent_t e = g_timer_pool.back();
    g_timer_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
}  // namespace

static void to_params(const dinox_gemm_args* a, GemmParams& p) {
  p.A = a->A; p.B = a->B; p.C = a->C;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
  p.batch = a->batch; p.strideA = a->strideA; p.strideB = a->strideB; p.strideC = a->strideC;
  p.transA = a->transA ? 1 : 0; p.transB = a->transB ? 1 : 0;
  p.in_dtype = a->in_dtype; p.out_dtype = a->out_dtype; p.epilogue = a->epilogue;
  p.alpha = a->alpha;
  p.bias = a->bias; p.residual = a->residual; p.ldr = a->ldr; p.aux = a->aux; p.ldaux = a->ldaux;
  p.colsum = a->colsum;
  p.ws = a->ws;
}

extern "C" int64_t dinox_gemm_ws_bytes(const dinox_gemm_args* a) {
  if (!a || a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch < 1) return 0;
  GemmParams p;
  to_params(a, p);
  return p.in_dtype == DINOX_BF16 ? gemm_bf16_ws_bytes(p) : 0;
}

extern "C" const char* dinox_gemm_kernel_name(const dinox_gemm_args* a) {
  if (!a) return "";
  GemmParams p;
  to_params(a, p);
  const char* v = gemm_variant_name(gemm_bf16_variant(p));
  return v ? v : "gemm_f32";
}

extern "C" int dinox_gemm(const dinox_gemm_args* a, void* stream) {
  DX_REQUIRE(a, DINOX_EINVAL, "gemm: null args");
  DX_REQUIRE(a->A && a->B && a->C, DINOX_EINVAL, "gemm: null operand");
  DX_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0 && a->batch >= 1, DINOX_EINVAL, "gemm: M=%lld N=%lld K=%lld batch=%lld",
             (long long)a->M, (long long)a->N, (long long)a->K, (long long)a->batch);
  DX_REQUIRE((a->in_dtype == DINOX_F32 || a->in_dtype == DINOX_BF16) && (a->out_dtype == DINOX_F32 || a->out_dtype == DINOX_BF16),
             DINOX_EINVAL, "gemm: dtype in=%d out=%d", a->in_dtype, a->out_dtype);
  DX_REQUIRE(a->lda >= (a->transA ? a->M : a->K) && a->ldb >= (a->transB ? a->N : a->K) && a->ldc >= a->N, DINOX_EINVAL,
             "gemm: leading dimension too small (lda=%lld ldb=%lld ldc=%lld)", (long long)a->lda, (long long)a->ldb, (long long)a->ldc);
  const int e = a->epilogue;
  DX_REQUIRE(!(e & DINOX_EPI_BIAS) || a->bias, DINOX_EINVAL, "gemm: BIAS without bias pointer");
  DX_REQUIRE(!(e & DINOX_EPI_RESIDUAL) || (a->residual && a->ldr >= a->N), DINOX_EINVAL, "gemm: RESIDUAL without residual/ldr");
  DX_REQUIRE(!(e & DINOX_EPI_DGELU) || (a->aux && a->ldaux >= a->N), DINOX_EINVAL, "gemm: DGELU without aux/ldaux");
  DX_REQUIRE(!(e & DINOX_EPI_GELU) || !a->aux || a->ldaux >= a->N, DINOX_EINVAL, "gemm: GELU aux ldaux too small");
  DX_REQUIRE(!((e & DINOX_EPI_GELU) && (e & DINOX_EPI_DGELU)), DINOX_EINVAL, "gemm: GELU and DGELU are exclusive");
  DX_REQUIRE(!(e & DINOX_EPI_ACCUM) || a->out_dtype == DINOX_F32, DINOX_EINVAL, "gemm: ACCUM needs fp32 C");
  DX_REQUIRE(!a->colsum || (a->transA && a->batch == 1), DINOX_EINVAL, "gemm: colsum needs transA=1 and batch=1");
  GemmParams p;
  to_params(a, p);
  hipStream_t st = as_stream(stream);
  // timing (dinox_gemm_timer_start .. stop): count every launch per (kernel, shape), bracket one in `every` with an event pair
  hipEvent_t e1 = nullptr;
  if (g_timer_on) {
    std::lock_guard<std::mutex> lk(g_timer_mu);
    if (g_timer_on) {
      const char* v = gemm_variant_name(gemm_bf16_variant(p));
      TimerRec& r = g_timer[TimerKey(v ? v : "gemm_f32", p.M, p.N, p.K, p.batch, p.epilogue, p.in_dtype, p.out_dtype,
                                     (p.aux && (p.epilogue & (DINOX_EPI_GELU | DINOX_EPI_DGELU))) ? 1 : 0, (p.batch > 1 && p.strideB == 0) ? 1 : 0)];
      r.launches++;
      ++g_timer_n;
      if (g_timer_every <= 1 || (((g_timer_n * 2654435761ull) & 0xffffffffull) * (uint64_t)g_timer_every >> 32) == 0) {
        hipEvent_t e0 = timer_event();
        e1 = timer_event();
        if (e0 && e1) {
          (void)hipEventRecord(e0, st);
          r.ev.emplace_back(e0, e1);
        } else {
          e1 = nullptr;
        }
      }
    }
  }
  int rc = DINOX_EUNSUPPORTED;
  if (p.in_dtype == DINOX_BF16) rc = launch_gemm_bf16(p, st);          // the TN kernel produces colsum itself
  if (rc == DINOX_EUNSUPPORTED) {
    // shape/layout outside the MFMA-bf16 kernel's envelope: exact-fp32 MFMA on the bf16 values.
    rc = 0;
    if (p.colsum)                                    // A is stored [K][M]: its column sums are the wanted vector
      rc = dinox_colsum(p.A, p.colsum, p.K, p.M, p.lda, p.in_dtype, (p.epilogue & DINOX_EPI_ACCUM) ? 1 : 0, stream);
    if (!rc) rc = launch_gemm_f32(p, st);
  }
  if (e1) (void)hipEventRecord(e1, st);
  return rc;
}

extern "C" int dinox_gemm_timer_start(int every) {
  std::lock_guard<std::mutex> lk(g_timer_mu);
  for (auto& kv : g_timer)
    for (auto& pr : kv.second.ev) {
      g_timer_pool.push_back(pr.first);
      g_timer_pool.push_back(pr.second);
    }
  g_timer.clear();
  g_timer_every = every < 1 ? 1 : every;
  g_timer_n = 0;
  g_timer_on = true;
  return 0;
}

extern "C" int64_t dinox_gemm_timer_stop(char* buf, int64_t buflen) {
  std::lock_guard<std::mutex> lk(g_timer_mu);
  g_timer_on = false;
  std::string out;
  char line[512];
  for (auto& kv : g_timer) {
    double ms = 0.0;
    int64_t timed = 0;
    for (auto& pr : kv.second.ev) {
      float t = 0.f;
      if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&t, pr.first, pr.second) == hipSuccess) {
        ms += t;
        ++timed;
      }
      g_timer_pool.push_back(pr.first);
      g_timer_pool.push_back(pr.second);
    }
    const TimerKey& k = kv.first;
    snprintf(line, sizeof line, "%s %lld %lld %lld %lld %d %d %d %d %d %lld %lld %.6f\n", std::get<0>(k).c_str(), (long long)std::get<1>(k),
             (long long)std::get<2>(k), (long long)std::get<3>(k), (long long)std::get<4>(k), std::get<5>(k), std::get<6>(k), std::get<7>(k),
             std::get<8>(k), std::get<9>(k), (long long)kv.second.launches, (long long)timed, ms);
    out += line;
  }
  g_timer.clear();
  if (!buf || (int64_t)out.size() + 1 > buflen) return -1;
  memcpy(buf, out.c_str(), out.size() + 1);
  return (int64_t)out.size();
}

extern "C" int dinox_colsum(const void* x, float* out, int64_t M, int64_t N, int64_t ldx, int dtype, int accumulate,
                            void* stream) {
  DX_REQUIRE(x && out, DINOX_EINVAL, "colsum: null pointer");
  DX_REQUIRE(M > 0 && N > 0 && ldx >= N, DINOX_EINVAL, "colsum: M=%lld N=%lld ldx=%lld", (long long)M, (long long)N, (long long)ldx);
  DX_REQUIRE(dtype == DINOX_F32 || dtype == DINOX_BF16, DINOX_EINVAL, "colsum: dtype %d", dtype);
  hipStream_t st = as_stream(stream);
  dim3 grid((unsigned)ceil_div(N, 64));
  if (dtype == DINOX_F32)
    hipLaunchKernelGGL((colsum_kernel<DINOX_F32>), grid, dim3(1024), 0, st, x, out, M, N, ldx, accumulate ? 1 : 0);
  else
    hipLaunchKernelGGL((colsum_kernel<DINOX_BF16>), grid, dim3(1024), 0, st, x, out, M, N, ldx, accumulate ? 1 : 0);
  return check_launch("colsum");
}
