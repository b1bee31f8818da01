// attention_common.h -- what the MFMA attention kernels share (attention_bf16.hip: whole-strip kernels, head size 64;
// attention_flash.hip: chunked kernels, image rows of DH = 64 / 96 / 128 columns).  Each piece is here once:
//   the LDS image layout at_off<DH> and its cooperative row load (load_image);
//   the fragment readers of that layout (frag_rows, frag_tr_perm; RowAddr / TrAddr + rd_rows / rd_tr where a K loop walks 32-row
//   tiles) -- every one of their transposed reads goes through ONE lo / hi pack, rd_tr_pair;
//   the accumulator helpers (zero16, acc_row, acc_as_a) and the global row-fragment loader (load_row_frags);
//   the grid of the persistent kernels (persist_grid).
//
// Conventions: v_mfma_f32_32x32x16_bf16.  Score tiles are computed TRANSPOSED (S^T = K . Q^T: keys in the accumulator rows, a query
// per lane) so that softmax statistics are lane-local and the accumulator is the next product's A operand as it stands, with no lane
// movement (guide section 3, "An accumulator tile as the next MFMA's operand"); the other operand is fetched in the matching
// permuted k order.  ONE LDS image layout serves row reads (ds_read_b128, MFMA A operands) and transposed reads (ds_read_b64_tr_b16,
// B operands whose reduction index runs down the rows) without bank conflicts: the 8-row x 32-column sub-tile image of
// cdna_hip_programming.md T10(a).
//
// The sharing rule is the one of gemm_pp_common.h: the device code stays byte-identical (tools/device_asm_diff.py).  Under that rule
// attn_fwd_bf16_persist and attn_qkv_fused_fwd keep their one-pass block, its address tables (addresses inside one image, where
// RowAddr / TrAddr hold offsets) and its row scaling written out: at ~250 registers their code changes with any helper that moves
// where an address or a product is computed ("Where the shared pieces live").
#pragma once
#include "common.h"

namespace dinox {

typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(3))) void at_lds_void;
typedef __attribute__((address_space(1))) const void at_gbl_void;
constexpr int AT_D = 64;                                      // head size of the whole-strip kernels

// ---------------------------------------------------------------- image layout
// byte offset of 16-B chunk ch (0 .. DH/8 - 1) of row r in a [rows][DH bf16] image: 8-row x 32-column sub-tiles of 512 B
template <int DH>
__device__ __forceinline__ int at_off(int r, int ch) {
  return (DH * 16) * (r >> 3) + 512 * (ch >> 2) + 64 * (r & 7) + 16 * ((ch & 3) ^ ((r >> 2) & 3));
}
__device__ __forceinline__ int img_off(int r, int ch) { return at_off<AT_D>(r, ch); }      // the 64-column (128-B row) form

// Cooperative load: rows [row0, row0 + rows) of a strided global matrix -> image rows 0 .. rows - 1 (rows >= n_valid and columns >= d
// are zero)
template <int DH>
__device__ __forceinline__ void load_image(char* __restrict__ img, const bf16_t* __restrict__ src, int64_t row_stride, int row0, int rows,
                                           int n_valid, int d) {
  constexpr int CH = DH / 8;
  for (int idx = threadIdx.x; idx < rows * CH; idx += blockDim.x) {
    const int r = idx / CH, ch = idx - r * CH;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row0 + r < n_valid && ch * 8 < d) v = *reinterpret_cast<const uint4*>(src + (int64_t)(row0 + r) * row_stride + ch * 8);
    *reinterpret_cast<uint4*>(img + at_off<DH>(r, ch)) = v;
  }
}

// ---------------------------------------------------------------- fragment readers
// Two transposed 8-byte LDS reads -> one B fragment.  The __restrict__ parameters are not decoration: after inlining they give the
// two reads alias-scope metadata, and hipcc's waitcnt insertion only falls back to "wait for every LDS-DMA in flight" (vmcnt(0),
// which in the persistent forward kernel means the NEXT pair's images, requested a moment earlier) for LDS reads that carry none.
__device__ __forceinline__ bf16x8 rd_tr_pair(const char* __restrict__ p0, const char* __restrict__ p1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p1);
  s16x8 v;
  v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3];
  v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
  return __builtin_bit_cast(bf16x8, v);
}

// A-operand fragment (standard k order): lane (row = l & 31, hl = l >> 5) gets img[row0 + row][16 ks + 8 hl + j], j < 8
template <int DH>
__device__ __forceinline__ bf16x8 frag_rows(const char* __restrict__ img, int row0, int ks, int lane) {
  return *reinterpret_cast<const bf16x8*>(img + at_off<DH>(row0 + (lane & 31), 2 * ks + (lane >> 5)));
}

// B-operand fragment in the PERMUTED k order that matches an accumulator tile used as the A operand:
// lane (col = l & 31, hl = l >> 5), element j  <-  img[row0 + 16 s + 8 (j >> 2) + 4 hl + (j & 3)][d0 + col]
template <int DH>
__device__ __forceinline__ bf16x8 frag_tr_perm(const char* __restrict__ img, int row0, int s, int d0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  const int q4 = i >> 2, p = i & 3, hl = g >> 1;
  const int ch = (d0 >> 3) + 2 * (g & 1) + (p >> 1);
  const int r0 = row0 + 16 * s + 4 * hl + q4;
  return rd_tr_pair(img + at_off<DH>(r0, ch) + 8 * (p & 1), img + at_off<DH>(r0 + 8, ch) + 8 * (p & 1));
}

// Per-lane constant parts of the fragment addresses of a 64-column image.  Tile t starts 4096 B after tile t - 1 (32 rows = four
// 1-KiB row groups; the swizzle terms depend on the row inside the tile only), so address = table entry + 4096 t: computed once per
// kernel, not per tile.  One table serves every image of a kernel (byte offsets, not addresses).
struct RowAddr {            // A-operand row reads: entry ks
  int off[4];
  __device__ __forceinline__ void init(int lane) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) off[ks] = img_off(lane & 31, 2 * ks + (lane >> 5));
  }
};
struct TrAddr {             // permuted-k transposed reads: entry [ss][dt][lo/hi]
  int off[2][2][2];
  __device__ __forceinline__ void init(int lane) {
    const int i = lane & 15, g = lane >> 4, q4 = i >> 2, pp = i & 3;
#pragma unroll
    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int ch = (dt * 32 >> 3) + 2 * (g & 1) + (pp >> 1);
        const int r0 = 16 * ss + 4 * (g >> 1) + q4;
        off[ss][dt][0] = img_off(r0, ch) + 8 * (pp & 1);
        off[ss][dt][1] = img_off(r0 + 8, ch) + 8 * (pp & 1);
      }
  }
};
__device__ __forceinline__ bf16x8 rd_rows(const char* img, const RowAddr& a, int ks, int t) {
  return *reinterpret_cast<const bf16x8*>(img + a.off[ks] + t * 4096);
}
__device__ __forceinline__ bf16x8 rd_tr(const char* img, const TrAddr& a, int ss, int dt, int t) {
  return rd_tr_pair(img + a.off[ss][dt][0] + t * 4096, img + a.off[ss][dt][1] + t * 4096);
}

// DH / 16 fragments of one global row of d valid elements: lane (row = l & 31, hl = l >> 5) takes columns 16 ks + 8 hl .. + 7 (zero
// past d)
template <int DH>
__device__ __forceinline__ void load_row_frags(bf16x8 (&f)[DH / 16], const bf16_t* __restrict__ rowp, int d, int lane) {
#pragma unroll
  for (int ks = 0; ks < DH / 16; ++ks) {
    const int c = 16 * ks + 8 * (lane >> 5);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (c < d) v = *reinterpret_cast<const uint4*>(rowp + c);
    f[ks] = __builtin_bit_cast(bf16x8, v);
  }
}

// ---------------------------------------------------------------- accumulator tiles
__device__ __forceinline__ void zero16(f32x16& x) {
#pragma unroll
  for (int e = 0; e < 16; ++e) x[e] = 0.f;
}

// row index inside a 32-row accumulator tile held by register e of lane-half hl
__device__ __forceinline__ int acc_row(int e, int hl) { return (e & 3) + 8 * (e >> 2) + 4 * hl; }

// accumulator registers [8 s, 8 s + 8) -> bf16 A fragment of k-step s
__device__ __forceinline__ bf16x8 acc_as_a(const f32x16& x, int s) {
  bf16x8 a;
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = (__bf16)x[8 * s + j];
  return a;
}

// ---------------------------------------------------------------- host: persistent grids
// Grid of a persistent attention kernel: one workgroup per resident slot of the chip, or one per (image, head) pair when there are
// fewer pairs.  Slots per CU: what 160 KiB of LDS and 8 waves admit (the kernels sit at ~250 registers: two waves per SIMD) -- one
// at 7 blocks (201 tokens); short sequences (the 41-token local crops: two waves, 41 KiB) get several: with one the chip ran half a
// wave per SIMD (113 us for 5 GFLOP at N = 41).
static int persist_grid(int64_t npairs, size_t lds_bytes, int waves) {
  const int by_lds = (int)((size_t)160 * 1024 / (lds_bytes ? lds_bytes : 1)), by_waves = 8 / (waves > 0 ? waves : 1);
  const int per_cu = by_lds < by_waves ? by_lds : by_waves;
  const int64_t slots = (int64_t)device_cu_count() * (per_cu < 1 ? 1 : per_cu);
  return (int)(npairs < slots ? npairs : slots);
}

}  // namespace dinox
