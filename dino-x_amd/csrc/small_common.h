// small_common.h -- what every file of small memory-bound kernels needs around its kernels: the 1-D grid size, the 16-byte alignment
// test, rows of fp32 / bf16 read and written 1 or 4 elements at a time, the two-way dtype launch and the one-workgroup strided sum.
// A new small-kernel file starts from these; the GEMM and attention kernels keep their own packs ("Where the shared pieces live").
#pragma once
#include "common.h"

namespace dinox {

// ---------------------------------------------------------------- host: launch geometry
// Workgroups of a grid-stride kernel over `total` items: ceil(total / threads) clamped to [1, cap].
static inline unsigned grid_1d(int64_t total, int threads, int64_t cap) {
  const int64_t b = ceil_div(total, threads);
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}

// Every pointer given is 16-byte aligned (a null pointer counts as aligned).
template <typename... P>
static inline bool aligned16(const P*... p) {
  return ((... | (uintptr_t)p) & 15) == 0;
}

// The two element types of the small kernels (what DX_LAUNCH_DT below can launch).
static inline bool dtype_ok(int dt) { return dt == DINOX_F32 || dt == DINOX_BF16; }

// ---------------------------------------------------------------- device: VW = 1 (any size) or 4 (16-byte fp32 / 8-byte bf16) row elements
template <int VW>
struct fvec {
  float e[VW];
};
template <int VW>
__device__ __forceinline__ fvec<VW> ld_f32(const float* p) {
  fvec<VW> r;
  if constexpr (VW == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.e[0] = q.x; r.e[1] = q.y; r.e[2] = q.z; r.e[3] = q.w;
  } else {
    r.e[0] = *p;
  }
  return r;
}
template <int VW>
__device__ __forceinline__ void st_f32(float* p, const fvec<VW>& v) {
  if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(v.e[0], v.e[1], v.e[2], v.e[3]);
  else *p = v.e[0];
}
template <int DT, int VW>
__device__ __forceinline__ fvec<VW> ld_dt(const void* p, int64_t i) {
  if constexpr (DT == DINOX_F32) {
    return ld_f32<VW>((const float*)p + i);
  } else {
    fvec<VW> r;
    if constexpr (VW == 4) {
      const uint2 w = *reinterpret_cast<const uint2*>((const bf16_t*)p + i);
      r.e[0] = __uint_as_float(w.x << 16); r.e[1] = __uint_as_float(w.x & 0xffff0000u);
      r.e[2] = __uint_as_float(w.y << 16); r.e[3] = __uint_as_float(w.y & 0xffff0000u);
    } else {
      r.e[0] = bf16_to_f32(((const bf16_t*)p)[i]);
    }
    return r;
  }
}
template <int DT, int VW>
__device__ __forceinline__ void st_dt(void* p, int64_t i, const fvec<VW>& v) {
  if constexpr (DT == DINOX_F32) {
    st_f32<VW>((float*)p + i, v);
  } else if constexpr (VW == 4) {
    uint2 w;
    w.x = (unsigned)f32_to_bf16(v.e[0]) | ((unsigned)f32_to_bf16(v.e[1]) << 16);
    w.y = (unsigned)f32_to_bf16(v.e[2]) | ((unsigned)f32_to_bf16(v.e[3]) << 16);
    *reinterpret_cast<uint2*>((bf16_t*)p + i) = w;
  } else {
    ((bf16_t*)p)[i] = f32_to_bf16(v.e[0]);
  }
}
template <int VW>
__device__ __forceinline__ fvec<VW> vadd(const fvec<VW>& a, const fvec<VW>& b) {
  fvec<VW> r;
#pragma unroll
  for (int i = 0; i < VW; ++i) r.e[i] = a.e[i] + b.e[i];
  return r;
}
template <int VW>
__device__ __forceinline__ fvec<VW> vzero() {
  fvec<VW> r;
#pragma unroll
  for (int i = 0; i < VW; ++i) r.e[i] = 0.f;
  return r;
}

// ---------------------------------------------------------------- host: kern<DT> / kern<DT, VW> by the runtime dtype
// Any dtype but DINOX_F32 / DINOX_BF16 makes the ENCLOSING function return DINOX_EINVAL.
#define DX_LAUNCH_DT(kern, dtype, grid, block, st, ...)                                                              \
  do {                                                                                                               \
    if ((dtype) == DINOX_F32) hipLaunchKernelGGL((kern<DINOX_F32>), grid, block, 0, st, __VA_ARGS__);                \
    else if ((dtype) == DINOX_BF16) hipLaunchKernelGGL((kern<DINOX_BF16>), grid, block, 0, st, __VA_ARGS__);         \
    else return ::dinox::fail(DINOX_EINVAL, #kern ": dtype %d", (int)(dtype));                                       \
  } while (0)

#define DX_LAUNCH_DT_VW(kern, dtype, vec, grid, block, st, ...)                                                      \
  do {                                                                                                               \
    if ((dtype) == DINOX_F32) {                                                                                      \
      if (vec) hipLaunchKernelGGL((kern<DINOX_F32, 4>), grid, block, 0, st, __VA_ARGS__);                            \
      else hipLaunchKernelGGL((kern<DINOX_F32, 1>), grid, block, 0, st, __VA_ARGS__);                                \
    } else if ((dtype) == DINOX_BF16) {                                                                              \
      if (vec) hipLaunchKernelGGL((kern<DINOX_BF16, 4>), grid, block, 0, st, __VA_ARGS__);                           \
      else hipLaunchKernelGGL((kern<DINOX_BF16, 1>), grid, block, 0, st, __VA_ARGS__);                               \
    } else {                                                                                                         \
      return ::dinox::fail(DINOX_EINVAL, #kern ": dtype %d", (int)(dtype));                                          \
    }                                                                                                                \
  } while (0)

// ---------------------------------------------------------------- device: one workgroup's sum of an array, in a fixed order
// Thread t adds x[t], x[t + blockDim.x], ... in ascending order, then block_sum (`red`: >= 16 floats of LDS); every thread gets the sum.
__device__ __forceinline__ float block_strided_sum(const float* __restrict__ x, int64_t n, float* red) {
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) a += x[i];
  return block_sum(a, red);
}
// The same over w[i] * x[i].
__device__ __forceinline__ float block_strided_sum(const float* __restrict__ x, const float* __restrict__ w, int64_t n, float* red) {
  float a = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += blockDim.x) a += w[i] * x[i];
  return block_sum(a, red);
}

}  // namespace dinox
