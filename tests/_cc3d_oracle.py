"""Connected components of one label volume [Z, H, W], the clean-up filter and the lesion-wise match counts, restated from the definitions
in include/dinox.h in plain NumPy / Python.  It calls no project code.

Two independent labellers: ``label_flood`` (breadth-first flood fill in raster order) and ``label_propagate`` (every voxel repeatedly takes
the minimum index over its same-class neighbourhood, with pointer jumping, until nothing changes).  tests/test_cclabel3d_cpu.py holds the
second to the first.  Both return (comp int32 [Z, H, W], area int32 [Z, H, W], ncomp int64 [C]) in the canonical form: comp = the index
(z H + y) W + x of the component's first voxel in raster order, -1 where the voxel is in no component; area = the voxel count at that
root, 0 elsewhere."""
from collections import deque
from itertools import product

import numpy as np

from _cc_oracle import bad_values, classes, overlap_counts  # noqa: F401  (shape-agnostic; re-exported for the tests)


def offsets(connectivity):
    """The neighbours of a voxel: they share a face (6), a face or an edge (18), a face, an edge or a corner (26)."""
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in product((-1, 0, 1), repeat=3) if 0 < abs(d[0]) + abs(d[1]) + abs(d[2]) <= reach]


def label_flood(vol, C, connectivity=26, mask=None):
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 3
    cl = classes(vol, C, None if mask is None else np.asarray(mask))
    Z, H, W = cl.shape
    comp = np.full((Z, H, W), -1, np.int32)
    area = np.zeros((Z, H, W), np.int32)
    ncomp = np.zeros(C, np.int64)
    offs = offsets(connectivity)
    cll = cl.tolist()
    for z, y, x in product(range(Z), range(H), range(W)):
        c = cll[z][y][x]
        if c < 0 or comp[z, y, x] >= 0:
            continue
        root = (z * H + y) * W + x                 # raster order: the first voxel of a component met is its smallest index
        comp[z, y, x] = root
        n, todo = 0, deque([(z, y, x)])
        while todo:
            pz, py, px = todo.popleft()
            n += 1
            for dz, dy, dx in offs:
                qz, qy, qx = pz + dz, py + dy, px + dx
                if 0 <= qz < Z and 0 <= qy < H and 0 <= qx < W and cll[qz][qy][qx] == c and comp[qz, qy, qx] < 0:
                    comp[qz, qy, qx] = root
                    todo.append((qz, qy, qx))
        area[z, y, x] = n
        ncomp[c] += 1
    return comp, area, ncomp


def label_propagate(vol, C, connectivity=26, mask=None):
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 3
    cl = classes(vol, C, None if mask is None else np.asarray(mask))
    Z, H, W = cl.shape
    n = Z * H * W
    lab = np.arange(n, dtype=np.int64).reshape(Z, H, W)
    pad_cl = np.pad(cl, 1, constant_values=-2)     # -2 matches no class, not even "none"
    offs = offsets(connectivity)
    while True:
        pad = np.pad(lab, 1, constant_values=n)
        new = lab.copy()
        for dz, dy, dx in offs:
            sl = (slice(1 + dz, 1 + dz + Z), slice(1 + dy, 1 + dy + H), slice(1 + dx, 1 + dx + W))
            new = np.where(pad_cl[sl] == cl, np.minimum(new, pad[sl]), new)
        new = new.ravel()[new]                     # pointer jumping: the label of my label's voxel (same component, never larger)
        if np.array_equal(new, lab):
            break
        lab = new
    comp = np.where(cl >= 0, lab, -1).astype(np.int32)
    area = np.zeros(n, np.int32)
    roots, sizes = np.unique(comp[comp >= 0], return_counts=True)
    area[roots] = sizes
    ncomp = np.bincount(vol.ravel()[roots], minlength=C).astype(np.int64)[:C]
    return comp, area.reshape(Z, H, W), ncomp


# ------------------------------------------------------------------------------------------ the filter
def cc_filter(vol, C, min_vox=None, keep_largest=False, first_class=1, connectivity=26, mask=None, label=label_flood):
    """out = vol where the voxel's component is kept, 0 where it is removed or the voxel is in none.  Classes < first_class: kept.
    Others: kept iff area >= min_vox (None: 1) and, with keep_largest, the largest of the class; equal areas: the smallest root."""
    vol = np.asarray(vol)
    comp, area, _ = label(vol, C, connectivity, mask)
    mv = 1 if min_vox is None else int(min_vox)
    roots = np.flatnonzero(area.ravel() > 0)
    cls, ar = vol.ravel()[roots], area.ravel()[roots]
    keep = set()
    for c in range(C):
        mine = [(int(a), int(r)) for a, r, k in zip(ar, roots, cls) if k == c]
        if not mine:
            continue
        if c < first_class:
            keep.update(r for _, r in mine)
            continue
        largest = min(mine, key=lambda t: (-t[0], t[1]))[1]
        keep.update(r for a, r in mine if a >= mv and (not keep_largest or r == largest))
    kept = np.isin(comp, np.fromiter(keep, np.int64, len(keep))) & (comp >= 0)
    out = np.zeros_like(vol)
    out[kept] = vol[kept]
    return out


# ------------------------------------------------------------------------------------------ lesion-wise counts
def lesion_counts(pred, gt, C, connectivity=26, overlap=(0, 1), min_vox=None, label=label_flood):
    """int64 [C, 4] = (n_gt, n_gt_hit, n_pred, n_pred_hit).  pred is labelled over the voxels gt does not ignore; inter of a component = its
    voxels with pred == gt that lie in a component on both sides; hit iff inter >= 1 and inter t_den >= t_num area; components with
    area < min_vox are not counted on their side (their voxels still overlap the other side's)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    t_num, t_den = overlap
    assert 0 <= t_num <= t_den and 0 < t_den < 1 << 20
    pc, pa, _ = label(pred, C, connectivity, gt)
    gc, ga, _ = label(gt, C, connectivity, None)
    mv = 1 if min_vox is None else int(min_vox)
    counts = np.zeros((C, 4), np.int64)
    both = (pc >= 0) & (gc >= 0) & (pred == gt)
    for side, (comp, area, lab) in enumerate(((gc, ga, gt), (pc, pa, pred))):
        inter = np.bincount(comp[both].ravel(), minlength=pred.size)
        for r in np.flatnonzero(area.ravel() > 0):
            a = int(area.ravel()[r])
            if a < mv:
                continue
            c = int(lab.ravel()[r])
            counts[c, 2 * side] += 1
            n = int(inter[r])
            if n >= 1 and n * t_den >= t_num * a:
                counts[c, 2 * side + 1] += 1
    return counts


def min_vox(min_volume_mm3, voxel_mm):
    """ceil(min_volume_mm3 / (s_z s_y s_x)) in float64."""
    s = [np.float64(v) for v in voxel_mm]
    return int(np.ceil(np.float64(min_volume_mm3) / (s[0] * s[1] * s[2])))


# ------------------------------------------------------------------------------------------ volumes the CPU and GPU tests share
def noise(shape, C=3, ignore=0.05, seed=0):
    """Uniform noise of C classes with a fraction ``ignore`` of 255."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, C, size=shape).astype(np.uint8)
    v[rng.random(shape) < ignore] = 255
    return v


def structured(shape, seed=0):
    """Three classes: a box of class 1, a diagonal slab of class 2 and sparse noise of all three on top."""
    Z, H, W = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(H), np.arange(W), indexing="ij")
    v = np.zeros(shape, np.uint8)
    v[(z >= Z // 4) & (y >= H // 4) & (y < 3 * H // 4 + 1) & (x >= W // 3)] = 1
    v[(x + y + z) % 7 == 0] = 2
    flip = rng.random(shape) < 0.15
    v[flip] = rng.integers(0, 3, size=int(flip.sum())).astype(np.uint8)
    return v


def mask_of(shape, seed=1):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.1, 255, 0).astype(np.uint8)


def checkerboard(shape):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return ((z + y + x) % 2).astype(np.uint8)


def serpentine(shape):
    """One one-voxel-wide path of class 1 through every slice.  An even slice holds a plane-filling serpentine (every other row, joined at
    alternating ends); an odd slice holds a single voxel that links its two neighbours, alternately at the path's far end and at its start.
    The path therefore runs against the raster order in every other even slice: long chains of roots.  The rest is class 0."""
    Z, H, W = shape
    plane = np.zeros((H, W), np.uint8)
    plane[0::2, :] = 1
    for y in range(1, H, 2):
        plane[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    k = (H - 1) // 2
    far = (2 * k, W - 1 if k % 2 == 0 else 0)      # where the path that starts at (0, 0) ends
    v = np.zeros(shape, np.uint8)
    for z in range(Z):
        if z % 2 == 0:
            v[z] = plane
        else:
            v[(z,) + (far if z % 4 == 1 else (0, 0))] = 1
    return v
