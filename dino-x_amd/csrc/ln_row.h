// ln_row.h -- the LayerNorm row arithmetic, ONE source for every kernel that runs it (layernorm.hip's kernels, the LN and LNB
// epilogues of gemm_bf16_pp384.hip, gemm_bf16_rowln.hip) and the float4 <-> four-bf16 conversion that goes with it.  The fused and
// the unfused paths must agree to the last bit ("LayerNorm row arithmetic"): the operation ORDER below is that contract.
// Statistics, reductions, row loops and prefetch stay in the kernels.  Device functions only, no state.
#pragma once
#include "common.h"

namespace dinox {

// ---------------------------------------------------------------- float4 <-> four bf16
// Four bf16 travel as a NATIVE vector: HIP's ushort4 is a struct, copied as one 64-bit integer when a function returns it, and hipcc then
// assembles every store with shifts and v_or_b32_sdwa where the native vector takes two v_cvt_pk_bf16_f32 and nothing else.
typedef bf16_t bf16x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bf16x4_t f32x4_to_bf16(const float4& v) { return bf16x4_t{f32_to_bf16(v.x), f32_to_bf16(v.y), f32_to_bf16(v.z), f32_to_bf16(v.w)}; }
__device__ __forceinline__ float4 bf16x4_to_f32(bf16x4_t p) { return make_float4(bf16_to_f32(p[0]), bf16_to_f32(p[1]), bf16_to_f32(p[2]), bf16_to_f32(p[3])); }
// four bf16 as two dwords (element 0 in the low half of .x): two shifts and two masks instead of four extractions
__device__ __forceinline__ float4 bf16x4_to_f32(const uint2& pk) {
  return make_float4(__uint_as_float(pk.x << 16), __uint_as_float(pk.x & 0xffff0000u), __uint_as_float(pk.y << 16), __uint_as_float(pk.y & 0xffff0000u));
}
// elements e .. e + 3 of an array of DT (e % 4 == 0, the array aligned for the vector access)
template <int DT>
__device__ __forceinline__ float4 load_row4(const void* p, int64_t e) {
  if constexpr (DT == DINOX_F32) return *reinterpret_cast<const float4*>((const float*)p + e);
  else return bf16x4_to_f32(*reinterpret_cast<const bf16x4_t*>((const bf16_t*)p + e));
}
// ... and their streaming store
template <int OUT_DT>
__device__ __forceinline__ void store_row4(void* y, int64_t e, const float4& o) {
  if constexpr (OUT_DT == DINOX_F32) store_stream(reinterpret_cast<float4*>((float*)y + e), o);
  else store_stream(reinterpret_cast<bf16x4_t*>((bf16_t*)y + e), f32x4_to_bf16(o));
}

// ---------------------------------------------------------------- forward: y = (v - mu) * rs * w + b
__device__ __forceinline__ float ln_scale_shift(float v, float mu, float rs, float w, float b) { return (v - mu) * rs * w + b; }
__device__ __forceinline__ float4 ln_scale_shift(const float4& v, float mu, float rs, const float4& w, const float4& b) {
  return make_float4(ln_scale_shift(v.x, mu, rs, w.x, b.x), ln_scale_shift(v.y, mu, rs, w.y, b.y), ln_scale_shift(v.z, mu, rs, w.z, b.z),
                     ln_scale_shift(v.w, mu, rs, w.w, b.w));
}

// ---------------------------------------------------------------- backward
// One float4 column group of one row: x_hat and g = dy gamma out; the column sums (aw += dy x_hat, ab += dy) and the row sums
// (s1 += sum g, s2 += sum g x_hat, pairwise inside the group) updated.
__device__ __forceinline__ void ln_bwd_accum(const float4& xv, const float4& d, const float4& wreg, float mu, float rs, float4& xh, float4& g,
                                             float4& aw, float4& ab, float& s1, float& s2) {
  xh = make_float4((xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs);
  g = make_float4(d.x * wreg.x, d.y * wreg.y, d.z * wreg.z, d.w * wreg.w);
  aw.x += d.x * xh.x; aw.y += d.y * xh.y; aw.z += d.z * xh.z; aw.w += d.w * xh.w;
  ab.x += d.x; ab.y += d.y; ab.z += d.z; ab.w += d.w;
  s1 += (g.x + g.y) + (g.z + g.w);
  s2 += (g.x * xh.x + g.y * xh.y) + (g.z * xh.z + g.w * xh.w);
}
// dx = rs (g - m1 - x_hat m2) + add, with m1 = mean(g), m2 = mean(g x_hat) of the row
__device__ __forceinline__ float ln_bwd_dx(float g, float xh, float rs, float m1, float m2, float add) { return rs * (g - m1 - xh * m2) + add; }
__device__ __forceinline__ float4 ln_bwd_dx(const float4& g, const float4& xh, float rs, float m1, float m2, const float4& add) {
  return make_float4(ln_bwd_dx(g.x, xh.x, rs, m1, m2, add.x), ln_bwd_dx(g.y, xh.y, rs, m1, m2, add.y), ln_bwd_dx(g.z, xh.z, rs, m1, m2, add.z),
                     ln_bwd_dx(g.w, xh.w, rs, m1, m2, add.w));
}
// elements e .. e + 3: dx in fp32 and, where asked for, its bf16 copy (both streaming)
__device__ __forceinline__ void ln_bwd_store(float* dx, void* dx_lowp, int64_t e, const float4& o) {
  store_row4<DINOX_F32>(dx, e, o);
  if (dx_lowp) store_row4<DINOX_BF16>(dx_lowp, e, o);
}

}  // namespace dinox
