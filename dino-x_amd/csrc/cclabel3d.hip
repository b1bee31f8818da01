// cclabel3d.hip -- connected components of ONE uint8 label volume [Z][H][W] with connectivity 6, 18 or 26: labelling in the canonical
// form of cclabel.hip (a component's label is its smallest linear index (z H + y) W + x), the clean-up filter and the lesion-wise match
// counts (definitions: include/dinox.h).
//
// Labelling is the union-find of cclabel.hip with the same invariant parent[i] <= i over the whole volume, Z H W <= 2^30.  Four launches:
//   1. cc_tile_kernel (cclabel.hip, `volume`): a workgroup per 32 x 32 tile of one slice, union-find in LDS with the in-plane part of the
//      connectivity (4 for 6; 8 for 18 and 26, whose in-plane neighbours share an edge or a corner alike); tile roots are written as
//      volume-wide indices.
//   2. cc_border_kernel (cclabel.hip, `volume`): unions across tile edges and corners inside each slice.
//   3. cc3d_zlink_kernel (here): a THREAD per voxel v with z >= 1 unites it with same-class neighbours in slice z - 1.  Only this backward
//      half of the neighbourhood is needed: the forward half is the backward half of the other voxel.  Offsets (dy, dx): connectivity 6
//      (0, 0); 18 adds (+-1, 0) and (0, +-1); 26 adds (+-1, +-1).
//        - If u = v - H W, directly above, has v's class, that one union is enough: every other candidate is an in-plane neighbour of u
//          under the in-plane connectivity of launches 1 and 2 (4 covers nothing more for 6, 8 covers all eight offsets), has u's class,
//          and is therefore joined to u already.
//        - And that union is skipped where the west neighbour w = v - 1 and its own u' = w - H W both carry the class too: v ~ w and u ~ u'
//          are in-plane edge unions, w ~ u' is made by w's thread (or, by the same argument, by the first voxel of the run), so v ~ u
//          follows.  One union per run of "same class as above" remains.
//        - Otherwise v is united with each candidate of its class.
//      Other threads change `parent` meanwhile: every access to it is an agent-scope atomic, loads included (cclabel.hip's header).
//   4. cc_flatten_kernel (cclabel.hip) over the volume as one array of Z H W voxels, after launch 3 has ended.
//
// Why every loop ends.  cc_find and cc_unite are cclabel.hip's, on strictly falling indices >= 0; the candidate loop of launch 3 runs over
// at most 8 fixed offsets; every other loop is a grid-stride loop over a count fixed at launch.  None waits for another wave.  No flag,
// no grid barrier, no host round trip, no floating point: equal inputs give equal bits.
#include "cc_common.h"

namespace dinox {

__global__ __launch_bounds__(CC_THREADS) void cc3d_zlink_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ mask, int* parent, int H, int W,
                                                                int C, int conn, int64_t hw, int64_t total) {
  // the backward neighbours other than (0, 0): four that share an edge with v (18 and 26), then four that share a corner (26)
  constexpr int DY[8] = {0, 0, -1, 1, -1, -1, 1, 1}, DX[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
  const int nnb = conn == 6 ? 0 : (conn == 18 ? 4 : 8);
  for (int64_t it = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * CC_THREADS) {
    const int64_t v = it + hw;                      // z >= 1; v < Z H W <= 2^30
    const int c = cc_class(labels, mask, v, C);
    if (c == CC_NONE) continue;
    const int64_t u = v - hw;
    const int p = (int)(v % hw), y = p / W, x = p % W;
    if (cc_class(labels, mask, u, C) == c) {
      if (x > 0 && cc_class(labels, mask, v - 1, C) == c && cc_class(labels, mask, u - 1, C) == c) continue;
      cc_unite<CC_AGENT>(parent, (int)v, (int)u);
      continue;
    }
    for (int k = 0; k < nnb; ++k) {
      const int yy = y + DY[k], xx = x + DX[k];
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const int64_t q = u + (int64_t)DY[k] * W + DX[k];
      if (cc_class(labels, mask, q, C) == c) cc_unite<CC_AGENT>(parent, (int)v, (int)q);
    }
  }
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// Z H W <= 2^30: every voxel index and every area fits int32, and 31 bits of the 64-bit tie key.
constexpr int64_t CC3D_MAX_VOXELS = (int64_t)1 << 30;
static_assert(CC3D_MAX_VOXELS <= ((int64_t)1 << (CC3D_KEY_BITS - 1)), "root and area must fit the tie key and int32");
static int cc3d_sizes(const char* what, int64_t Z, int H, int W, int C) {
  return cc_check_sizes(what, 'Z', Z, CC3D_MAX_VOXELS, "Z H W <= 2^30; label a longer series in pieces", H, W, C);
}

// label: parent [Z][H][W] int32.  filter: best [C] uint64.  match: ip, ig [Z][H][W] int32 each.
extern "C" int64_t dinox_cc3d_ws_bytes(int64_t Z, int H, int W, int C) {
  return cc_broken_limit(Z, CC3D_MAX_VOXELS, H, W, C) ? 0 : 8 * Z * (int64_t)H * W + 8 * (int64_t)C;
}

extern "C" int dinox_cc3d_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t Z,
                                int H, int W, int C, int connectivity, void* stream) {
  DX_REQUIRE(labels && comp && area && ncomp && bad && ws, DINOX_EINVAL, "cc3d_label: null pointer");
  int rc = cc3d_sizes("cc3d_label", Z, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, DINOX_EINVAL, "cc3d_label: connectivity=%d (6, 18 or 26)", connectivity);
  hipStream_t st = as_stream(stream);
  const int64_t hw = (int64_t)H * W;
  int* parent = (int*)ws;
  rc = cc_zero(ncomp, C * (int64_t)sizeof(int64_t), st, "cc3d_label");
  if (rc) return rc;
  rc = cc_run_planes(labels, mask, parent, area, bad, Z, H, W, C, connectivity == 6 ? 4 : 8, 1, st, "cc3d_label");
  if (rc) return rc;
  if (Z > 1) {
    const int64_t total = (Z - 1) * hw;
    hipLaunchKernelGGL(cc3d_zlink_kernel, dim3(grid_1d(total, CC_THREADS, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, mask, parent, H, W, C, connectivity,
                       hw, total);
    rc = check_launch("cc3d_label (z links)");
    if (rc) return rc;
  }
  return cc_run_flatten(labels, parent, comp, area, ncomp, 1, Z * hw, C, st, "cc3d_label");
}

extern "C" int dinox_cc3d_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, int min_vox, const uint8_t* y, uint8_t* out,
                                 int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int c0, int keep_largest, void* stream) {
  DX_REQUIRE(labels && comp && area && out && ws, DINOX_EINVAL, "cc3d_filter: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "cc3d_filter: y and counts go together (both or neither)");
  const int rc = cc3d_sizes("cc3d_filter", Z, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(min_vox >= 0, DINOX_EINVAL, "cc3d_filter: min_vox=%d (>= 0)", min_vox);
  DX_REQUIRE(c0 >= 0 && c0 <= C, DINOX_EINVAL, "cc3d_filter: c0=%d (0 <= c0 <= C = %d)", c0, C);
  return cc_run_filter(labels, comp, area, nullptr, min_vox, y, out, counts, ws, 1, Z * (int64_t)H * W, C, c0, keep_largest ? 1 : 0, CC3D_KEY_BITS,
                       as_stream(stream), "cc3d_filter");
}

extern "C" int dinox_cc3d_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                                const int32_t* gt_area, int min_vox, int64_t* counts, void* ws, int64_t Z, int H, int W, int C, int t_num, int t_den,
                                void* stream) {
  DX_REQUIRE(pred && pred_comp && pred_area && gt && gt_comp && gt_area && counts && ws, DINOX_EINVAL, "cc3d_match: null pointer");
  const int rc = cc3d_sizes("cc3d_match", Z, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(min_vox >= 0, DINOX_EINVAL, "cc3d_match: min_vox=%d (>= 0)", min_vox);
  DX_REQUIRE(t_den > 0 && t_den < (1 << 20) && t_num >= 0 && t_num <= t_den, DINOX_EINVAL,
             "cc3d_match: overlap %d/%d (0 <= t_num <= t_den, 0 < t_den < 2^20)", t_num, t_den);
  return cc_run_match(pred, pred_comp, pred_area, gt, gt_comp, gt_area, nullptr, min_vox, counts, ws, 1, Z * (int64_t)H * W, C, t_num, t_den,
                      as_stream(stream), "cc3d_match");
}
