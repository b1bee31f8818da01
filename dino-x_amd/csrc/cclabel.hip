// cclabel.hip -- connected components of a uint8 label map: labelling in a canonical form, the clean-up filter (minimum area, largest
// component) and lesion-wise match counts (definitions: include/dinox.h).
//
// Labelling is union-find over the pixels of one image with the invariant parent[i] <= i, so a component's root is its smallest index
// y W + x, which is the canonical label.  Three launches:
//   1. cc_tile_kernel: a WORKGROUP per 32 x 32 tile.  Union-find in LDS on tile-local indices (raster order inside the tile, so the
//      local order is the global order), then every pixel writes its tile root as a global index into `parent`; -1 = in no component.
//   2. cc_border_kernel: a THREAD per pixel on a tile edge unites it with its west / north (and, connectivity 8, north-west / north-east)
//      neighbours that lie in another tile.  Other workgroups change `parent` meanwhile, so EVERY access to it is an agent-scope
//      atomic, loads included (a plain load may be served from an L1 or an L2 that another XCD's store never reached).
//   3. cc_flatten_kernel (after launch 2 has ended: the kernel boundary orders the rest): every pixel finds its root; area and ncomp
//      are integer atomics, reduced inside the wave first (cc_wave_add) and inside the workgroup (LDS) first.
// A diagonal pair needs no union of its own where an edge neighbour of both has the same class (the two edge unions imply it), which
// leaves the north-west union for "north and west both differ" and the north-east union for "north differs".
//
// Why every loop ends.  cc_find walks x -> parent[x] only while parent[x] < x: x falls strictly and is >= 0.  cc_unite repeats only after
// an atomicMin that returned a value below the root it was applied to, so the pair (a, b) falls strictly.  cc_wave_add retires at
// least one of 64 lanes per pass.  Every other loop is a grid-stride loop over a count fixed at launch.  None of them waits for another
// wave: what other waves do can only lower parents, which shortens the walks.  No flag, no grid barrier, no host round trip, no
// floating point: equal inputs give equal bits, and an image's outputs do not depend on what else is in the batch.
// A label is compared with class numbers and 255 only; it indexes nothing before `< C` has been tested.
//
// The primitives (cc_find, cc_unite, cc_wave_add, cc_class) and the constants live in cc_common.h.  The launches are grouped into the stages
// cc_run_planes / cc_run_flatten / cc_run_filter / cc_run_match, which cclabel3d.hip runs again on a volume: there the B images are the
// slices of one array, `volume` makes launches 1 and 2 write volume-wide indices into ONE parent array, and the per-pixel stages see the
// volume as a single array of Z H W elements.
#include "cc_common.h"

namespace dinox {

// ---------------------------------------------------------------- 1: union-find of one tile in LDS
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ mask, int* __restrict__ parent,
                                                             int* __restrict__ area, unsigned long long* __restrict__ bad, int H, int W, int C, int conn,
                                                             int volume, int ntx, int nty, int64_t ntiles) {
  __shared__ int par[CC_TPX];
  __shared__ uint8_t cls[CC_TPX];
  const int64_t hw = (int64_t)H * W;
  unsigned nbad = 0;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {        // uniform per workgroup: the barriers inside are reached by all
    const int x0 = (int)(t % ntx) * CC_TILE, y0 = (int)((t / ntx) % nty) * CC_TILE;
    const int64_t img = (t / ((int64_t)ntx * nty)) * hw;
#pragma unroll
    for (int j = 0; j < CC_TPX / CC_THREADS; ++j) {
      const int l = j * CC_THREADS + (int)threadIdx.x;
      const int y = y0 + l / CC_TILE, x = x0 + l % CC_TILE;
      int c = CC_NONE;
      if (y < H && x < W) {
        const int64_t i = img + (int64_t)y * W + x;
        c = cc_class(labels, mask, i, C);
        nbad += (c == CC_NONE && labels[i] != 255 && !(mask && mask[i] == 255)) ? 1u : 0u;
        area[i] = 0;
      }
      cls[l] = (uint8_t)c;
      par[l] = l;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_TPX / CC_THREADS; ++j) {
      const int l = j * CC_THREADS + (int)threadIdx.x;
      const int ly = l / CC_TILE, lx = l % CC_TILE, c = cls[l];
      if (c == CC_NONE) continue;
      const bool w = lx > 0 && cls[l - 1] == c, n = ly > 0 && cls[l - CC_TILE] == c;
      if (w) cc_unite<CC_WG>(par, l, l - 1);
      if (n) cc_unite<CC_WG>(par, l, l - CC_TILE);
      if (conn == 8 && ly > 0 && !n) {
        if (lx > 0 && !w && cls[l - CC_TILE - 1] == c) cc_unite<CC_WG>(par, l, l - CC_TILE - 1);
        if (lx < CC_TILE - 1 && cls[l - CC_TILE + 1] == c) cc_unite<CC_WG>(par, l, l - CC_TILE + 1);
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_TPX / CC_THREADS; ++j) {
      const int l = j * CC_THREADS + (int)threadIdx.x;
      const int y = y0 + l / CC_TILE, x = x0 + l % CC_TILE;
      if (y >= H || x >= W) continue;
      int r = -1;
      if (cls[l] != CC_NONE) {
        const int rl = cc_find<CC_WG>(par, l);
        r = (volume ? (int)img : 0) + (y0 + rl / CC_TILE) * W + x0 + rl % CC_TILE;   // volume: B H W <= 2^30
      }
      parent[img + (int64_t)y * W + x] = r;
    }
    __syncthreads();                                                // the next tile reuses par and cls
  }
  if (nbad) atomicAdd(bad, (unsigned long long)nbad);
}

// ---------------------------------------------------------------- 2: unions across tile edges and corners
// Per image the candidates are: the nA pixels of the rows y = 32 k (k >= 1), the nB pixels of the columns x = 32 k (k >= 1) and, for
// connectivity 8, the nB pixels of the columns x = 32 k - 1 (their north-east neighbour is in the next tile).  Each looks at its west,
// north, north-west and north-east neighbours and unites with those in ANOTHER tile; a pair seen from two candidate sets is united twice,
// which changes nothing.
__global__ __launch_bounds__(CC_THREADS) void cc_border_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ mask, int* parent, int H,
                                                               int W, int C, int conn, int volume, int nA, int nB, int per, int64_t total) {
  const int64_t hw = (int64_t)H * W;
  for (int64_t it = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * CC_THREADS) {
    const int64_t img = (it / per) * hw;
    int r = (int)(it % per), y, x;
    if (r < nA) {
      y = (r / W + 1) * CC_TILE, x = r % W;
    } else if (r < nA + nB) {
      r -= nA;
      x = (r / H + 1) * CC_TILE, y = r % H;
    } else {
      r -= nA + nB;
      x = (r / H + 1) * CC_TILE - 1, y = r % H;
    }
    const uint8_t* lab = labels + img;
    const uint8_t* msk = mask ? mask + img : nullptr;
    int* L = volume ? parent : parent + img;
    const int i = y * W + x;
    const int g = (volume ? (int)img : 0) + i;      // the pixel as launch 1 numbered it
    const int c = cc_class(lab, msk, i, C);
    if (c == CC_NONE) continue;
    const bool w = x > 0 && cc_class(lab, msk, i - 1, C) == c, n = y > 0 && cc_class(lab, msk, i - W, C) == c;
    const bool xedge = x % CC_TILE == 0, yedge = y % CC_TILE == 0;
    if (w && xedge) cc_unite<CC_AGENT>(L, g, g - 1);
    if (n && yedge) cc_unite<CC_AGENT>(L, g, g - W);
    if (conn == 8 && y > 0 && !n) {
      if (x > 0 && !w && (xedge || yedge) && cc_class(lab, msk, i - W - 1, C) == c) cc_unite<CC_AGENT>(L, g, g - W - 1);
      if (x + 1 < W && (x % CC_TILE == CC_TILE - 1 || yedge) && cc_class(lab, msk, i - W + 1, C) == c) cc_unite<CC_AGENT>(L, g, g - W + 1);
    }
  }
}

// ---------------------------------------------------------------- 3: every pixel its root; area at the roots; components per class
// A work item is one chunk of 1024 consecutive pixels of ONE image.  The walks still halve paths (a long chain of tile roots is
// walked by many pixels), so parent is read and written with agent-scope atomics here as well.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const uint8_t* __restrict__ labels, int* parent, int* __restrict__ comp, int* area,
                                                                unsigned long long* __restrict__ ncomp, int64_t hw, int C, int64_t nchunk, int64_t nitems) {
  __shared__ unsigned nc[SEG_MAX_CLASSES];
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t b = item / nchunk, img = b * hw;
    const int i0 = (int)(item % nchunk) * CC_CHUNK;
    if (threadIdx.x < SEG_MAX_CLASSES) nc[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < CC_CHUNK / CC_THREADS; ++j) {
      const int i = i0 + j * CC_THREADS + (int)threadIdx.x;
      int r = -1;
      if (i < hw) {
        if (cc_ld<CC_AGENT>(parent + img + i) >= 0) r = cc_find<CC_AGENT>(parent + img, i);
        comp[img + i] = r;
        const int c = labels[img + i];
        if (r == i && c < C) atomicAdd(&nc[c], 1u);
      }
      cc_wave_add(area + img, r, r >= 0);
    }
    __syncthreads();
    if ((int)threadIdx.x < C && nc[threadIdx.x]) atomicAdd(&ncomp[b * C + threadIdx.x], (unsigned long long)nc[threadIdx.x]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- filter: the largest component per (image, class), then the kept pixels
__global__ __launch_bounds__(CC_THREADS) void cc_best_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ area,
                                                             unsigned long long* __restrict__ best, int64_t hw, int C, int c0, int key_bits,
                                                             int64_t total) {
  for (int64_t g = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x; g < total; g += (int64_t)gridDim.x * CC_THREADS) {
    const int a = area[g];
    if (a <= 0) continue;                           // not a root
    const int c = labels[g];
    if (c < c0 || c >= C) continue;
    const unsigned long long root = (unsigned long long)(g % hw);
    atomicMax(&best[(g / hw) * C + c], ((unsigned long long)a << key_bits) | (((1ull << key_bits) - 1) - root));
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const uint8_t* __restrict__ labels, const int* __restrict__ comp, const int* __restrict__ area,
                                                               const int* __restrict__ min_px, int min_all, const unsigned long long* __restrict__ best,
                                                               const uint8_t* __restrict__ y, uint8_t* __restrict__ out,
                                                               unsigned long long* __restrict__ counts, int64_t hw, int C, int c0, int keep_largest,
                                                               int key_bits, int64_t nchunk, int64_t nitems) {
  const int kmask = (int)((1ull << key_bits) - 1);  // key_bits <= 31
  constexpr int CP = SEG_MAX_CLASSES;
  __shared__ unsigned cnt[3 * CP + 1];               // true positives, predicted, labelled per class; bad values of y
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t b = item / nchunk, img = b * hw;
    const int i0 = (int)(item % nchunk) * CC_CHUNK;
    if (y) {
      for (int t = threadIdx.x; t < 3 * CP + 1; t += CC_THREADS) cnt[t] = 0;
      __syncthreads();
    }
    const int mp = min_px ? min_px[b] : min_all;
#pragma unroll
    for (int j = 0; j < CC_CHUNK / CC_THREADS; ++j) {
      const int i = i0 + j * CC_THREADS + (int)threadIdx.x;
      if (i >= hw) continue;
      const int r = comp[img + i], c = labels[img + i];
      int o = 0;
      if (r >= 0 && r < hw && c < C) {
        bool keep = c < c0;
        if (!keep) {
          keep = area[img + r] >= mp;
          if (keep && keep_largest) keep = (int)(best[b * C + c] & (unsigned long long)kmask) == kmask - r;
        }
        o = keep ? c : 0;
      }
      out[img + i] = (uint8_t)o;
      if (y) {
        const int lab = y[img + i];
        if (lab == 255) continue;
        if (lab >= C) {
          atomicAdd(&cnt[3 * CP], 1u);
          continue;
        }
        if (o == lab) atomicAdd(&cnt[o], 1u);
        atomicAdd(&cnt[CP + o], 1u);
        atomicAdd(&cnt[2 * CP + lab], 1u);
      }
    }
    if (y) {                                        // uniform
      __syncthreads();
      for (int t = threadIdx.x; t < 3 * C; t += CC_THREADS) {
        const unsigned v = cnt[(t / C) * CP + t % C];
        if (v) atomicAdd(&counts[t], (unsigned long long)v);
      }
      if (threadIdx.x == 0 && cnt[3 * CP]) atomicAdd(&counts[3 * C], (unsigned long long)cnt[3 * CP]);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------- match: overlap per component, then the lesion counts
// ip / ig [B][H][W] int32, zeroed: at a root, the number of pixels of its component with pred == gt inside a component on both sides.
__global__ __launch_bounds__(CC_THREADS) void cc_inter_kernel(const uint8_t* __restrict__ pred, const int* __restrict__ pcomp, const uint8_t* __restrict__ gt,
                                                              const int* __restrict__ gcomp, int* ip, int* ig, int64_t hw, int64_t nchunk, int64_t nitems) {
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t img = (item / nchunk) * hw;
    const int i0 = (int)(item % nchunk) * CC_CHUNK;
#pragma unroll
    for (int j = 0; j < CC_CHUNK / CC_THREADS; ++j) {
      const int i = i0 + j * CC_THREADS + (int)threadIdx.x;
      int rp = -1, rg = -1;
      if (i < hw) {
        rp = pcomp[img + i], rg = gcomp[img + i];
        if (rp < 0 || rp >= hw || rg < 0 || rg >= hw || pred[img + i] != gt[img + i]) rp = rg = -1;
      }
      cc_wave_add(ip + img, rp, rp >= 0);
      cc_wave_add(ig + img, rg, rg >= 0);
    }
  }
}

// counts[B][C][4] = (n_gt, n_gt_hit, n_pred, n_pred_hit): roots with area >= min_px; hit: inter >= 1 and inter t_den >= t_num area.
__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(const uint8_t* __restrict__ pred, const int* __restrict__ parea, const uint8_t* __restrict__ gt,
                                                              const int* __restrict__ garea, const int* __restrict__ ip, const int* __restrict__ ig,
                                                              const int* __restrict__ min_px, int min_all, unsigned long long* __restrict__ counts, int64_t hw, int C,
                                                              int t_num, int t_den, int64_t nchunk, int64_t nitems) {
  __shared__ unsigned cnt[4 * SEG_MAX_CLASSES];
  for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
    const int64_t b = item / nchunk, img = b * hw;
    const int i0 = (int)(item % nchunk) * CC_CHUNK;
    cnt[threadIdx.x] = 0;                           // 256 threads, 4 * 64 counters
    __syncthreads();
    const int mp = min_px ? min_px[b] : min_all;
#pragma unroll
    for (int j = 0; j < CC_CHUNK / CC_THREADS; ++j) {
      const int i = i0 + j * CC_THREADS + (int)threadIdx.x;
      if (i >= hw) continue;
#pragma unroll
      for (int side = 0; side < 2; ++side) {        // 0: gt, 1: pred
        const int a = side ? parea[img + i] : garea[img + i];
        if (a <= 0 || a < mp) continue;             // not a root, or too small to be a lesion
        const int c = side ? pred[img + i] : gt[img + i];
        if (c >= C) continue;
        const int n = side ? ip[img + i] : ig[img + i];
        atomicAdd(&cnt[c * 4 + 2 * side], 1u);
        if (n >= 1 && (int64_t)n * t_den >= (int64_t)t_num * a) atomicAdd(&cnt[c * 4 + 2 * side + 1], 1u);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 * C && cnt[threadIdx.x]) atomicAdd(&counts[b * C * 4 + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------- host
static_assert(CC_THREADS == 4 * SEG_MAX_CLASSES, "cc_count_kernel zeroes one counter per thread");
static_assert((int64_t)CC_MAX_SIDE * CC_MAX_SIDE <= (1 << CC_KEY_BITS), "root and area must fit the tie key");

static int cc_check(const char* what, const char* stage) {
  char msg[96];
  snprintf(msg, sizeof msg, "%s (%s)", what, stage);
  return check_launch(msg);
}

int cc_run_planes(const uint8_t* labels, const uint8_t* mask, int* parent, int32_t* area, int64_t* bad, int64_t B, int H, int W, int C, int conn, int volume,
                  hipStream_t st, const char* what) {
  int rc = cc_zero(bad, sizeof(int64_t), st, what);
  if (rc) return rc;
  const int ntx = (int)ceil_div(W, CC_TILE), nty = (int)ceil_div(H, CC_TILE);
  const int64_t ntiles = B * ntx * nty;
  hipLaunchKernelGGL(cc_tile_kernel, dim3(grid_1d(ntiles, 1, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, mask, parent, area, (unsigned long long*)bad, H,
                     W, C, conn, volume, ntx, nty, ntiles);
  rc = cc_check(what, "tiles");
  if (rc) return rc;
  const int nA = (nty - 1) * W, nB = (ntx - 1) * H, per = nA + nB + (conn == 8 ? nB : 0);
  if (per > 0) {
    const int64_t total = B * per;
    hipLaunchKernelGGL(cc_border_kernel, dim3(grid_1d(total, CC_THREADS, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, mask, parent, H, W, C, conn, volume,
                       nA, nB, per, total);
    rc = cc_check(what, "borders");
  }
  return rc;
}

int cc_run_flatten(const uint8_t* labels, int* parent, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t B, int64_t n, int C, hipStream_t st,
                   const char* what) {
  const int64_t nchunk = ceil_div(n, CC_CHUNK), nitems = B * nchunk;
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_1d(nitems, 1, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, parent, comp, area,
                     (unsigned long long*)ncomp, n, C, nchunk, nitems);
  return cc_check(what, "flatten");
}

int cc_run_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, int min_all, const uint8_t* y, uint8_t* out,
                  int64_t* counts, void* ws, int64_t B, int64_t n, int C, int c0, int keep_largest, int key_bits, hipStream_t st, const char* what) {
  unsigned long long* best = (unsigned long long*)ws;
  int rc;
  if (y) {
    rc = cc_zero(counts, (3 * C + 1) * (int64_t)sizeof(int64_t), st, what);
    if (rc) return rc;
  }
  if (keep_largest) {
    rc = cc_zero(best, B * C * (int64_t)sizeof(int64_t), st, what);
    if (rc) return rc;
    hipLaunchKernelGGL(cc_best_kernel, dim3(grid_1d(B * n, CC_THREADS, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, area, best, n, C, c0, key_bits, B * n);
    rc = cc_check(what, "largest");
    if (rc) return rc;
  }
  const int64_t nchunk = ceil_div(n, CC_CHUNK), nitems = B * nchunk;
  hipLaunchKernelGGL(cc_filter_kernel, dim3(grid_1d(nitems, 1, CC_GRID_CAP)), dim3(CC_THREADS), 0, st, labels, comp, area, min_px, min_all, best, y, out,
                     (unsigned long long*)counts, n, C, c0, keep_largest, key_bits, nchunk, nitems);
  return check_launch(what);
}

int cc_run_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp, const int32_t* gt_area,
                 const int32_t* min_px, int min_all, int64_t* counts, void* ws, int64_t B, int64_t n, int C, int t_num, int t_den, hipStream_t st,
                 const char* what) {
  int* ip = (int*)ws;
  int* ig = ip + B * n;
  int rc = cc_zero(ws, 2 * B * n * (int64_t)sizeof(int), st, what);
  if (rc) return rc;
  rc = cc_zero(counts, B * C * 4 * (int64_t)sizeof(int64_t), st, what);
  if (rc) return rc;
  const int64_t nchunk = ceil_div(n, CC_CHUNK), nitems = B * nchunk;
  const unsigned grid = grid_1d(nitems, 1, CC_GRID_CAP);
  hipLaunchKernelGGL(cc_inter_kernel, dim3(grid), dim3(CC_THREADS), 0, st, pred, pred_comp, gt, gt_comp, ip, ig, n, nchunk, nitems);
  rc = cc_check(what, "overlap");
  if (rc) return rc;
  hipLaunchKernelGGL(cc_count_kernel, dim3(grid), dim3(CC_THREADS), 0, st, pred, pred_area, gt, gt_area, ip, ig, min_px, min_all,
                     (unsigned long long*)counts, n, C, t_num, t_den, nchunk, nitems);
  return cc_check(what, "counts");
}

}  // namespace dinox

using namespace dinox;

// ---------------------------------------------------------------- entry points
// B H W < 2^31: every pixel index of an image fits int32 (and 20 bits: H, W <= 1024), every batch offset int64.
constexpr int64_t CC_MAX_PIXELS = ((int64_t)1 << 31) - 1;
static int cc_sizes(const char* what, int64_t B, int H, int W, int C) {
  return cc_check_sizes(what, 'B', B, CC_MAX_PIXELS, "B H W < 2^31; cut a longer batch in pieces", H, W, C);
}

// label: parent [B][H][W] int32.  filter: best [B][C] uint64.  match: ip, ig [B][H][W] int32 each.
extern "C" int64_t dinox_cc_ws_bytes(int64_t B, int H, int W, int C) {
  return cc_broken_limit(B, CC_MAX_PIXELS, H, W, C) ? 0 : 8 * B * (int64_t)H * W + 8 * B * C;
}

extern "C" int dinox_cc_label(const uint8_t* labels, const uint8_t* mask, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t* bad, void* ws, int64_t B,
                              int H, int W, int C, int connectivity, void* stream) {
  DX_REQUIRE(labels && comp && area && ncomp && bad && ws, DINOX_EINVAL, "cc_label: null pointer");
  int rc = cc_sizes("cc_label", B, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(connectivity == 4 || connectivity == 8, DINOX_EINVAL, "cc_label: connectivity=%d (4 or 8)", connectivity);
  hipStream_t st = as_stream(stream);
  rc = cc_zero(ncomp, B * C * (int64_t)sizeof(int64_t), st, "cc_label");
  if (rc) return rc;
  rc = cc_run_planes(labels, mask, (int*)ws, area, bad, B, H, W, C, connectivity, 0, st, "cc_label");
  return rc ? rc : cc_run_flatten(labels, (int*)ws, comp, area, ncomp, B, (int64_t)H * W, C, st, "cc_label");
}

extern "C" int dinox_cc_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, const uint8_t* y, uint8_t* out,
                               int64_t* counts, void* ws, int64_t B, int H, int W, int C, int c0, int keep_largest, void* stream) {
  DX_REQUIRE(labels && comp && area && out && ws, DINOX_EINVAL, "cc_filter: null pointer");
  DX_REQUIRE((y == nullptr) == (counts == nullptr), DINOX_EINVAL, "cc_filter: y and counts go together (both or neither)");
  const int rc = cc_sizes("cc_filter", B, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(c0 >= 0 && c0 <= C, DINOX_EINVAL, "cc_filter: c0=%d (0 <= c0 <= C = %d)", c0, C);
  return cc_run_filter(labels, comp, area, min_px, 1, y, out, counts, ws, B, (int64_t)H * W, C, c0, keep_largest ? 1 : 0, CC_KEY_BITS, as_stream(stream),
                       "cc_filter");
}

extern "C" int dinox_cc_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp,
                              const int32_t* gt_area, const int32_t* min_px, int64_t* counts, void* ws, int64_t B, int H, int W, int C, int t_num,
                              int t_den, void* stream) {
  DX_REQUIRE(pred && pred_comp && pred_area && gt && gt_comp && gt_area && counts && ws, DINOX_EINVAL, "cc_match: null pointer");
  const int rc = cc_sizes("cc_match", B, H, W, C);
  if (rc) return rc;
  DX_REQUIRE(t_den > 0 && t_den < (1 << 20) && t_num >= 0 && t_num <= t_den, DINOX_EINVAL,
             "cc_match: overlap %d/%d (0 <= t_num <= t_den, 0 < t_den < 2^20)", t_num, t_den);
  return cc_run_match(pred, pred_comp, pred_area, gt, gt_comp, gt_area, min_px, 1, counts, ws, B, (int64_t)H * W, C, t_num, t_den, as_stream(stream),
                      "cc_match");
}
