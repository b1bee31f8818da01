// cc_common.h -- what the two connected-component files share: cclabel.hip (a batch of independent [H][W] images) and cclabel3d.hip (one
// [Z][H][W] volume).  The union-find primitives on an int32 parent array with parent[i] <= i, the wave-reduced integer add, the class of
// a pixel, the launch constants, the size limits both families' entry points check, and the stage launchers that cclabel.hip defines and
// cclabel3d.hip runs again on a volume.
//
// Why every loop here ends is argued at each function; none waits for another wave (cclabel.hip's header has the whole argument).
#pragma once
#include "small_common.h"
#include "kernels.h"

namespace dinox {

constexpr int CC_TILE = 32;                        // tile side: 1024 local parents (4 KiB) + 1 KiB of classes in LDS
constexpr int CC_TPX = CC_TILE * CC_TILE;
constexpr int CC_THREADS = 256;                    // four pixels of a tile, or of a chunk, per thread
constexpr int CC_CHUNK = 4 * CC_THREADS;           // pixels of one image per work item of the per-pixel kernels
constexpr int CC_MAX_SIDE = 1024;                  // a root index y W + x and an area both fit 20 bits beside each other in the 64-bit tie key
constexpr int CC_NONE = 255;                       // class of a pixel in no component
constexpr int64_t CC_GRID_CAP = 1 << 20;           // workgroups per launch; the kernels stride over what is left
constexpr int CC_KEY_BITS = 20;                    // images: root < 2^20 and area <= 2^20, area << 20 | (2^20 - 1 - root) orders "larger, then lower root"
constexpr int CC3D_KEY_BITS = 31;                  // volumes: root < 2^30 and area <= 2^30, area << 31 | (2^31 - 1 - root), the same order

#define CC_AGENT __HIP_MEMORY_SCOPE_AGENT
#define CC_WG __HIP_MEMORY_SCOPE_WORKGROUP

template <int SCOPE>
__device__ __forceinline__ int cc_ld(int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}
template <int SCOPE>
__device__ __forceinline__ int cc_min(int* p, int v) {
  return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
}

// Root of x, halving the path on the way (a parent is only ever replaced by a smaller member of the same component).
// Ends: the loop runs only while p < x (unsigned: a negative p stops it too) and then x = p, so x falls strictly.
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* L, int x) {
  int p = cc_ld<SCOPE>(L + x);
  while ((unsigned)p < (unsigned)x) {
    const int gp = cc_ld<SCOPE>(L + p);
    if ((unsigned)gp < (unsigned)p) cc_min<SCOPE>(L + x, gp);
    x = p;
    p = gp;
  }
  return x;
}

// Join the components of a and b: the larger root gets the smaller as its parent.  If another wave re-parented that root first, the
// atomicMin returns what it wrote (old < a): L[a] is now min(old, b), and old and b are still to be joined -- the next pass.
// Ends: a pass that does not return replaces a by old < a while b does not rise; both are >= 0.
template <int SCOPE>
__device__ __forceinline__ void cc_unite(int* L, int a, int b) {
  for (;;) {
    a = cc_find<SCOPE>(L, a);
    b = cc_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = cc_min<SCOPE>(L + a, b);
    if (old >= a) return;                           // a was still a root (old == a; parent <= child rules out old > a)
    a = old;
  }
}

// base[key] += the number of lanes of this wave with `todo` and this key, one atomic per distinct key.  All 64 lanes call it together.
// Ends: uniform control flow; every pass clears at least bit `src` of rem.
__device__ __forceinline__ void cc_wave_add(int* base, int key, bool todo) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long rem = __ballot(todo);
  while (rem) {
    const int src = __ffsll((long long)rem) - 1;
    const int lead = __shfl(key, src);
    const unsigned long long m = __ballot(todo && key == lead);
    if (lane == src) atomicAdd(base + lead, (int)__popcll(m));
    rem &= ~m;
  }
}

// Class of pixel i of one image: 0 .. C - 1, or CC_NONE (masked out, 255, or a bad value).
__device__ __forceinline__ int cc_class(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ msk, int64_t i, int C) {
  if (msk && msk[i] == 255) return CC_NONE;
  const int v = lab[i];
  return v < C ? v : CC_NONE;
}

static inline int cc_zero(void* p, int64_t bytes, hipStream_t st, const char* what) {
  const hipError_t e = hipMemsetAsync(p, 0, (size_t)bytes, st);
  return e == hipSuccess ? 0 : fail((int)e, "%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
}

// ---------------------------------------------------------------- host: the size limits of `lead` images, or slices, of H x W pixels in C classes
// Said once: 0 inside all of them, else the number of the first one broken.  max_px bounds lead and lead H W.
static inline int cc_broken_limit(int64_t lead, int64_t max_px, int H, int W, int C) {
  if (!(H >= 1 && H <= CC_MAX_SIDE && W >= 1 && W <= CC_MAX_SIDE)) return 1;
  if (!(C >= 2 && C <= SEG_MAX_CLASSES)) return 2;
  if (!(lead >= 1 && lead <= max_px && lead * H * W <= max_px)) return 3;
  return 0;
}
// 0, or entry `what`'s refusal of the first broken limit.  `letter` names the leading extent ('B', 'Z') and `tail` says its limit.
static inline int cc_check_sizes(const char* what, char letter, int64_t lead, int64_t max_px, const char* tail, int H, int W, int C) {
  switch (cc_broken_limit(lead, max_px, H, W, C)) {
    case 1: return fail(DINOX_EINVAL, "%s: H=%d W=%d (1 <= H, W <= %d)", what, H, W, CC_MAX_SIDE);
    case 2: return fail(DINOX_EINVAL, "%s: C=%d (2 <= C <= %d)", what, C, SEG_MAX_CLASSES);
    case 3: return fail(DINOX_EINVAL, "%s: %c=%lld (%c >= 1 and %s)", what, letter, (long long)lead, letter, tail);
  }
  return 0;
}

// ---------------------------------------------------------------- the stages (cclabel.hip), for B images or, `volume`, the B slices of one volume
// `what` names the calling entry in error messages.  conn is the in-plane connectivity, 4 or 8.
// cc_run_planes: zeroes bad, the tile launch and the tile-border launch.  Afterwards parent holds, for every pixel in a component, a member
//   of its in-plane component that is <= the pixel: as an index inside its image, or, `volume`, as an index into the whole volume (then
//   B H W <= 2^30 and parent is one array for all slices).
// cc_run_flatten: every pixel of B arrays of n elements finds its root; comp, area, ncomp as dinox.h defines them.  The caller has zeroed
//   ncomp[B][C] on the stream, before the first launch.
// cc_run_filter / cc_run_match: the launches of dinox_cc_filter / dinox_cc_match over B arrays of n elements with the tie key of `key_bits`;
//   where min_px is NULL every array's minimum area is min_all.
int cc_run_planes(const uint8_t* labels, const uint8_t* mask, int* parent, int32_t* area, int64_t* bad, int64_t B, int H, int W, int C, int conn, int volume,
                  hipStream_t st, const char* what);
int cc_run_flatten(const uint8_t* labels, int* parent, int32_t* comp, int32_t* area, int64_t* ncomp, int64_t B, int64_t n, int C, hipStream_t st,
                   const char* what);
int cc_run_filter(const uint8_t* labels, const int32_t* comp, const int32_t* area, const int32_t* min_px, int min_all, const uint8_t* y, uint8_t* out,
                  int64_t* counts, void* ws, int64_t B, int64_t n, int C, int c0, int keep_largest, int key_bits, hipStream_t st, const char* what);
int cc_run_match(const uint8_t* pred, const int32_t* pred_comp, const int32_t* pred_area, const uint8_t* gt, const int32_t* gt_comp, const int32_t* gt_area,
                 const int32_t* min_px, int min_all, int64_t* counts, void* ws, int64_t B, int64_t n, int C, int t_num, int t_den, hipStream_t st,
                 const char* what);

}  // namespace dinox
