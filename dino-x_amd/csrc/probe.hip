// probe.hip -- loss, gradient and probabilities of a multinomial logistic (softmax) probe in one pass over the rows.  With the intercept as
// the last column of theta [C][D+1] and x~_i = [x_i, 1]:
//   z_ic = theta_c . x~_i     p_i = softmax(z_i)     loss = sum_i (logsumexp(z_i) - z_i,label_i)     grad_c = sum_i (p_ic - [label_i == c]) x~_i
// One call is one evaluation of the L-BFGS fit in dinox.probes.logistic_probe (the reference fits scikit-learn's LogisticRegression on the
// host, scripts/evaluate_panorgan.py:375-379); the predict form (no loss, no gradient) gives the test probabilities.
//
// A workgroup stages 32 rows once, as [32][D], and uses that image twice on the exact-fp32 MFMA (the intercept stays out of the products:
// it is added to the logits in the softmax step, and its gradient is the column sum of R):
//   logits   out[class][row], K = D: the classes (padded to 32, rows of zeros) are the A operand, held in registers for the whole launch;
//            the four waves each take a quarter of K and the quarters are added in wave order.  A lane reads four consecutive d of its row
//            with one 16-byte LDS load (the order of K inside the MFMA chain is free as long as both operands agree); the row pitch is
//            4 mod 64 floats, so the 16 lanes of a load group cover the 64 banks once.
//   softmax  eight lanes per row, four classes each, in log-sum-exp form (max, exp, sum, log: no overflow at any logit).
//   grad     out[class][d] = R^T X, K = the 32 rows: R = p - onehot (zero for rows past N and rows whose label is outside [0, C)) goes to
//            LDS as the A operand, the B operand is the row image again (rows that do not count are zeroed in it first, so that a
//            non-finite value in such a row cannot reach the gradient as 0 * inf).  A wave owns the same quarter of the columns as in the logits and
//            keeps its accumulators over all row blocks of the workgroup.
// The workgroups walk the row blocks round-robin (block b belongs to workgroup b mod G, G a pure function of N), write one fp32 partial
// gradient and one double partial loss each, and a second launch adds the partials in ascending workgroup order in double.
// No atomics, plain stores: two runs give identical bits, and the probabilities do not depend on which outputs were asked for.
// A label is only ever compared with class numbers.  Non-finite inputs propagate; no address or loop depends on a value.
#include "common.h"

namespace dinox {

constexpr int PB_ROWS = 32, PB_THREADS = 256, PB_CMAX = 32, PB_DMAX = 1024;
constexpr int PB_PP = 33;                        // pitch of the logit quarters [wave][row][class]: a wave's 32 rows land on 32 banks
constexpr int PB_RP = 36;                        // pitch of R [row][class]
constexpr int64_t PB_GROUPS = 512;               // workgroups of a launch (two resident per CU at D = 384)

static inline int64_t pb_groups(int64_t N) {
  const int64_t blocks = ceil_div(N, (int64_t)PB_ROWS);
  return blocks < PB_GROUPS ? blocks : PB_GROUPS;
}
static inline int pb_colsz(int64_t D) { return (int)((D + 3) / 4 * 4); }                 // columns of the row image (x, zeros), whole quads
static inline int pb_pitch(int64_t D) { return (pb_colsz(D) - 4 + 63) / 64 * 64 + 4; }   // smallest pitch >= colsz that is 4 mod 64
static inline size_t pb_lds_bytes(int64_t D) {
  return ((size_t)PB_ROWS * pb_pitch(D) + 4 * PB_ROWS * PB_PP + PB_ROWS * PB_RP + PB_ROWS) * sizeof(float);
}

// NB: 128-column quarters per wave -- a wave owns columns [wave 32 NB, (wave + 1) 32 NB) of x, D <= 128 NB (D = 384: NB = 3, no idle column).
template <int NB, bool VEC>
__global__ __launch_bounds__(PB_THREADS, NB <= 4 ? 2 : 1) void probe_sweep(const float* __restrict__ x, int64_t ldx,
                                                                          const int32_t* __restrict__ label, int64_t N, int D, int C,
                                                                          const float* __restrict__ theta, int want_grad,
                                                                          float* __restrict__ prob, double* __restrict__ ws_loss,
                                                                          float* __restrict__ ws_grad) {
  extern __shared__ __attribute__((aligned(16))) float pb_lds[];
  const int ncols = D + 1, colsz = (D + 3) / 4 * 4, pitch = (colsz - 4 + 63) / 64 * 64 + 4;
  float* Xs = pb_lds;                            // [32][pitch]
  float* Ps = Xs + PB_ROWS * pitch;              // [4][32][PB_PP]
  float* Rs = Ps + 4 * PB_ROWS * PB_PP;          // [32][PB_RP]
  float* rowloss = Rs + PB_ROWS * PB_RP;         // [32]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 31, h = lane >> 5;
  const int dbase = wv * 32 * NB;

  // this lane's share of theta: class c, d = dbase + 8 m + 4 h + s for K step 4 m + s (the lanes h = 0 / 1 supply k = 0 / 1 of a step)
  float th[4 * NB][4];
#pragma unroll
  for (int m = 0; m < 4 * NB; ++m)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int d = dbase + 8 * m + 4 * h + s;
      th[m][s] = (c < C && d < D) ? theta[(int64_t)c * ncols + d] : 0.f;
    }
  f32x16 gacc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) gacc[nb][e] = 0.f;
  double loss_acc = 0.0;                         // thread 0
  float bias_acc = 0.f;                          // threads 0..31: the intercept gradient of class tid, sum_i R[i][tid]
  float bias[4];                                 // the intercepts of this thread's four classes in the softmax step
#pragma unroll
  for (int q = 0; q < 4; ++q) bias[q] = (4 * (tid & 7) + q < C) ? theta[(int64_t)(4 * (tid & 7) + q) * ncols + D] : 0.f;

  const int64_t blocks = ceil_div(N, (int64_t)PB_ROWS);
  for (int64_t blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const int64_t row0 = blk * PB_ROWS;
    // ---- stage [32][colsz]: eight threads per row, 128 contiguous bytes per step
    {
      const int r = tid >> 3;
      const int64_t gr = row0 + r;
      const float* xr = x + gr * ldx;
      for (int q = tid & 7; 4 * q < colsz; q += 8) {
        const int d0 = 4 * q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gr < N) {
          if (VEC && d0 + 4 <= D) {
            v = *reinterpret_cast<const f32x4*>(xr + d0);
          } else {
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
              if (d0 + cc < D) v[cc] = xr[d0 + cc];
          }
        }
        *reinterpret_cast<f32x4*>(Xs + r * pitch + d0) = v;
      }
    }
    __syncthreads();

    // ---- logits: this wave's quarter of K
    {
      f32x16 z;
#pragma unroll
      for (int e = 0; e < 16; ++e) z[e] = 0.f;
#pragma unroll
      for (int m = 0; m < 4 * NB; ++m) {
        const int d0 = dbase + 8 * m + 4 * h;
        f32x4 xb = {0.f, 0.f, 0.f, 0.f};
        if (d0 < colsz) xb = *reinterpret_cast<const f32x4*>(Xs + c * pitch + d0);
#pragma unroll
        for (int s = 0; s < 4; ++s) z = __builtin_amdgcn_mfma_f32_32x32x2f32(th[m][s], xb[s], z, 0, 0, 0);
      }
      // z[e] = quarter logit of (class (e & 3) + 8 (e >> 2) + 4 h, row c)
#pragma unroll
      for (int e = 0; e < 16; ++e) Ps[(wv * PB_ROWS + c) * PB_PP + (e & 3) + 8 * (e >> 2) + 4 * h] = z[e];
    }
    __syncthreads();

    // ---- softmax of a row on eight lanes, four classes each
    {
      const int r = tid >> 3, sub = tid & 7;
      const int64_t gr = row0 + r;
      const int lab = gr < N ? label[gr] : -1;
      float zc[4], mx = -INFINITY;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cls = 4 * sub + q;
        const float* p = Ps + r * PB_PP + cls;
        zc[q] = (((p[0] + p[PB_ROWS * PB_PP]) + p[2 * PB_ROWS * PB_PP]) + p[3 * PB_ROWS * PB_PP]) + bias[q];
        if (cls < C) mx = fmaxf(mx, zc[q]);
        else zc[q] = -INFINITY;
      }
      // (fmaxf drops a NaN: fold it back in so that a NaN logit makes the row NaN rather than vanish)
      float bad = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (4 * sub + q < C && zc[q] != zc[q]) bad = zc[q];
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float ob = __shfl_xor(bad, o, 64);
        if (ob != ob) bad = ob;
      }
      if (bad != bad) mx = bad;
      if (mx == INFINITY || mx == -INFINITY) mx = (mx > 0.f) ? mx : 0.f;     // all -inf: exp(-inf - 0) = 0, sum 0, NaN row; +inf: inf - inf = NaN
      float ex[4], sum = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ex[q] = (4 * sub + q < C) ? expf(zc[q] - mx) : 0.f;
        sum += ex[q];
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o, 64);
      const float lse = mx + logf(sum), inv = 1.f / sum;
      float mine = 0.f;
      int hit = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cls = 4 * sub + q;
        const float p = ex[q] * inv;
        if (prob && gr < N && cls < C) prob[gr * C + cls] = p;
        const bool is = cls < C && cls == lab;
        if (is) {
          mine = lse - zc[q];
          hit = 1;
        }
        ex[q] = p - (is ? 1.f : 0.f);
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        mine += __shfl_xor(mine, o, 64);         // one lane at most holds a non-zero term: exact
        hit |= __shfl_xor(hit, o, 64);
      }
      const bool counts = hit && gr < N;
#pragma unroll
      for (int q = 0; q < 4; ++q) Rs[r * PB_RP + 4 * sub + q] = (counts && 4 * sub + q < C) ? ex[q] : 0.f;
      if (sub == 0) rowloss[r] = counts ? mine : 0.f;
      // a row that does not count leaves the image too: 0 * x would turn a non-finite x into a NaN in the gradient
      if (want_grad && !counts)
        for (int d0 = 4 * sub; d0 < colsz; d0 += 32) *reinterpret_cast<f32x4*>(Xs + r * pitch + d0) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    // ---- gradient of this block: K = the 32 rows
    if (want_grad) {
      if (tid == 0)
        for (int r = 0; r < PB_ROWS; ++r) loss_acc += (double)rowloss[r];
      if (tid < PB_CMAX) {
        float sr = 0.f;
        for (int r = 0; r < PB_ROWS; ++r) sr += Rs[r * PB_RP + tid];
        bias_acc += sr;
      }
      float ra[16];
#pragma unroll
      for (int s = 0; s < 16; ++s) ra[s] = Rs[(2 * s + h) * PB_RP + c];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const int d = dbase + nb * 32 + c;
        const bool in = d < colsz;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
          const float xb = in ? Xs[(2 * s + h) * pitch + d] : 0.f;
          gacc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra[s], xb, gacc[nb], 0, 0, 0);
        }
      }
    }
    __syncthreads();                             // the next block's staging overwrites the images
  }

  if (want_grad) {
    // gacc[nb][e] = partial of (class (e & 3) + 8 (e >> 2) + 4 h, column dbase + nb 32 + c)
    float* out = ws_grad + (int64_t)blockIdx.x * C * ncols;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int cls = (e & 3) + 8 * (e >> 2) + 4 * h, d = dbase + nb * 32 + c;
        if (cls < C && d < D) out[(int64_t)cls * ncols + d] = gacc[nb][e];
      }
    if (tid < C) out[(int64_t)tid * ncols + D] = bias_acc;
    if (tid == 0) ws_loss[blockIdx.x] = loss_acc;
  }
}

// ------------------------------------------------------------------------------------------ sum of the workgroups' partials
__global__ __launch_bounds__(256) void probe_finish(const double* __restrict__ ws_loss, const float* __restrict__ ws_grad, int64_t groups,
                                                    int64_t count, double* __restrict__ loss, double* __restrict__ grad) {
  const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (item < count) {
    if (!grad) return;
    double s = 0.0;
    for (int64_t g = 0; g < groups; ++g) s += (double)ws_grad[g * count + item];           // ascending workgroup: a fixed order
    grad[item] = s;
  } else if (item == count && loss) {
    double s = 0.0;
    for (int64_t g = 0; g < groups; ++g) s += ws_loss[g];
    loss[0] = s;
  }
}

template <int NB, bool VEC>
static int probe_launch(const float* x, int64_t ldx, const int32_t* label, int64_t N, int D, int C, const float* theta, int want_grad, float* prob,
                        double* ws_loss, float* ws_grad, hipStream_t st) {
  const size_t lds = pb_lds_bytes(D);
  if (int rc = reserve_lds((const void*)probe_sweep<NB, VEC>, lds, "probe_sweep")) return rc;
  hipLaunchKernelGGL((probe_sweep<NB, VEC>), dim3((unsigned)pb_groups(N)), dim3(PB_THREADS), lds, st, x, ldx, label, N, D, C, theta, want_grad, prob,
                     ws_loss, ws_grad);
  return check_launch("probe_sweep");
}

}  // namespace dinox

using namespace dinox;

extern "C" int64_t dinox_softmax_probe_ws_bytes(int64_t N, int64_t D, int C) {
  if (N < 1 || D < 1 || D > PB_DMAX || C < 2 || C > PB_CMAX) return 0;        // what dinox_softmax_probe refuses
  return pb_groups(N) * (8 + (int64_t)C * (D + 1) * 4);                       // a double loss and an fp32 [C][D + 1] gradient per workgroup
}

extern "C" int dinox_softmax_probe(const float* x, int64_t ldx, const int32_t* label, int64_t N, int64_t D, int C, const float* theta, double* loss,
                                   double* grad, float* prob, void* ws, void* stream) {
  DX_REQUIRE(C >= 2 && C <= PB_CMAX, DINOX_EINVAL, "softmax_probe: C=%d outside [2, %d]", C, PB_CMAX);
  DX_REQUIRE(N >= 1 && D >= 1 && D <= PB_DMAX && ldx >= D, DINOX_EINVAL, "softmax_probe: N=%lld D=%lld (1..%d) ldx=%lld", (long long)N,
             (long long)D, PB_DMAX, (long long)ldx);
  DX_REQUIRE(x && label && theta && ws, DINOX_EINVAL, "softmax_probe: null pointer");
  DX_REQUIRE(loss || grad || prob, DINOX_EINVAL, "softmax_probe: null pointer (no output asked for)");
  const int64_t groups = pb_groups(N);
  double* ws_loss = (double*)ws;
  float* ws_grad = (float*)(ws_loss + groups);
  const int want_grad = (loss || grad) ? 1 : 0;
  const bool vec = (uintptr_t)x % 16 == 0 && ldx % 4 == 0;
  const int nb = (int)ceil_div(D, (int64_t)128);
  hipStream_t st = as_stream(stream);
  int rc;
#define PROBE(NBV) \
  rc = vec ? probe_launch<NBV, true>(x, ldx, label, N, (int)D, C, theta, want_grad, prob, ws_loss, ws_grad, st) \
           : probe_launch<NBV, false>(x, ldx, label, N, (int)D, C, theta, want_grad, prob, ws_loss, ws_grad, st)
  if (nb <= 1) PROBE(1);
  else if (nb <= 2) PROBE(2);
  else if (nb <= 3) PROBE(3);
  else if (nb <= 4) PROBE(4);
  else PROBE(8);
#undef PROBE
  if (rc) return rc;
  if (!want_grad) return 0;
  const int64_t count = (int64_t)C * (D + 1);
  hipLaunchKernelGGL(probe_finish, dim3((unsigned)ceil_div(count + 1, (int64_t)256)), dim3(256), 0, st, (const double*)ws_loss, (const float*)ws_grad,
                     groups, count, loss, grad);
  return check_launch("probe_finish");
}
