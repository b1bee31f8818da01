"""Connected components of a label map, the clean-up filter, the lesion-wise match counts and the lesion metrics, restated from the
definitions in include/dinox.h in plain NumPy / Python.  It calls no project code.

Two labellers: ``label_flood`` (breadth-first flood fill; small maps) and ``label_runs`` (union-find over the runs of every row; the
1024 x 1024 map).  tests/test_cclabel_cpu.py holds the second to the first.  Both return, for uint8 maps [B, H, W],
(comp int32 [B, H, W], area int32 [B, H, W], ncomp int64 [B, C]) in the canonical form: comp = the index y W + x of the component's first
pixel in raster order, -1 where the pixel is in no component; area = the pixel count at that root pixel, 0 elsewhere."""
from collections import deque

import numpy as np

EDGE = ((-1, 0), (0, -1), (0, 1), (1, 0))
CORNER = ((-1, -1), (-1, 1), (1, -1), (1, 1))


def classes(labels, C, mask=None):
    """int32 map: the class 0 .. C - 1 of a pixel, -1 where it is in no component (mask == 255, or a label >= C)."""
    cl = labels.astype(np.int32)
    cl[labels >= C] = -1
    if mask is not None:
        cl[mask == 255] = -1
    return cl


def bad_values(labels, C, mask=None):
    """The number of labels >= C other than 255 at pixels the mask does not exclude."""
    bad = (labels >= C) & (labels != 255)
    if mask is not None:
        bad &= mask != 255
    return int(bad.sum())


def _offsets(connectivity):
    assert connectivity in (4, 8)
    return EDGE if connectivity == 4 else EDGE + CORNER


def _flood_one(cl, C, connectivity):
    H, W = cl.shape
    comp = np.full((H, W), -1, np.int32)
    area = np.zeros((H, W), np.int32)
    ncomp = np.zeros(C, np.int64)
    offs = _offsets(connectivity)
    for y in range(H):
        for x in range(W):
            c = cl[y, x]
            if c < 0 or comp[y, x] >= 0:
                continue
            root = y * W + x                       # raster order: the first pixel of a component met is its smallest index
            comp[y, x] = root
            n, todo = 0, deque([(y, x)])
            while todo:
                py, px = todo.popleft()
                n += 1
                for dy, dx in offs:
                    qy, qx = py + dy, px + dx
                    if 0 <= qy < H and 0 <= qx < W and cl[qy, qx] == c and comp[qy, qx] < 0:
                        comp[qy, qx] = root
                        todo.append((qy, qx))
            area[y, x] = n
            ncomp[c] += 1
    return comp, area, ncomp


def _runs_one(cl, C, connectivity):
    H, W = cl.shape
    d = 1 if connectivity == 8 else 0
    assert connectivity in (4, 8)
    parent, first, length, rows = [], [], [], []   # per run: union-find parent (always the smaller id), first pixel, length; runs per row

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    prev = []
    for y in range(H):
        row = cl[y]
        cuts = np.flatnonzero(np.diff(row)) + 1
        starts = np.concatenate(([0], cuts))
        ends = np.concatenate((cuts, [W]))
        cur = []
        for s, e in zip(starts.tolist(), ends.tolist()):
            c = int(row[s])
            if c < 0:
                continue
            rid = len(parent)
            parent.append(rid)
            first.append(y * W + s)
            length.append(e - s)
            cur.append((s, e, c, rid))
            for ps, pe, pc, pid in prev:
                if pc == c and ps < e + d and pe > s - d:
                    a, b = find(pid), find(rid)
                    if a != b:
                        parent[max(a, b)] = min(a, b)      # run ids follow raster order of their first pixels
        rows.append(cur)
        prev = cur
    comp = np.full((H, W), -1, np.int32)
    area = np.zeros((H, W), np.int32)
    ncomp = np.zeros(C, np.int64)
    total = {}
    for y, cur in enumerate(rows):
        for s, e, c, rid in cur:
            r = find(rid)
            comp[y, s:e] = first[r]
            total[r] = total.get(r, 0) + length[rid]
            if r == rid:
                ncomp[c] += 1
    for r, n in total.items():
        area[first[r] // W, first[r] % W] = n
    return comp, area, ncomp


def _label(one, labels, C, connectivity, mask):
    labels = np.asarray(labels)
    assert labels.dtype == np.uint8 and labels.ndim == 3
    out = [one(classes(labels[b], C, None if mask is None else np.asarray(mask)[b]), C, connectivity) for b in range(labels.shape[0])]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def label_flood(labels, C, connectivity=8, mask=None):
    return _label(_flood_one, labels, C, connectivity, mask)


def label_runs(labels, C, connectivity=8, mask=None):
    return _label(_runs_one, labels, C, connectivity, mask)


# ------------------------------------------------------------------------------------------ the filter
def cc_filter(labels, C, min_px=None, keep_largest=False, first_class=1, connectivity=8, mask=None, label=label_flood):
    """out = labels where the pixel's component is kept, 0 where it is removed or the pixel is in none.  Classes < first_class: kept.
    Others: kept iff area >= min_px[b] and, with keep_largest, the largest of (b, class); equal areas: the smallest root."""
    labels = np.asarray(labels)
    comp, area, _ = label(labels, C, connectivity, mask)
    B, H, W = labels.shape
    out = np.zeros_like(labels)
    for b in range(B):
        mp = 1 if min_px is None else int(min_px[b])
        roots = np.flatnonzero(area[b].ravel() > 0)
        cls = labels[b].ravel()[roots]
        ar = area[b].ravel()[roots]
        keep = set()
        for c in range(C):
            mine = [(int(a), int(r)) for a, r, k in zip(ar, roots, cls) if k == c]
            if not mine:
                continue
            if c < first_class:
                keep.update(r for _, r in mine)
                continue
            largest = min(mine, key=lambda t: (-t[0], t[1]))[1]
            keep.update(r for a, r in mine if a >= mp and (not keep_largest or r == largest))
        kept = np.isin(comp[b], np.fromiter(keep, np.int64, len(keep))) & (comp[b] >= 0)
        out[b][kept] = labels[b][kept]
    return out


def overlap_counts(out, y, C):
    """dinox_seg_predict's counts of a label map against targets: int64 [3, C] = true positives, predicted, labelled over y != 255 (and
    y < C), then the number of y values >= C other than 255."""
    out, y = np.asarray(out), np.asarray(y)
    valid = y < C
    counts = np.zeros((3, C), np.int64)
    for c in range(C):
        counts[0, c] = (valid & (out == c) & (y == c)).sum()
        counts[1, c] = (valid & (out == c)).sum()
        counts[2, c] = (valid & (y == c)).sum()
    return counts, int(((y >= C) & (y != 255)).sum())


# ------------------------------------------------------------------------------------------ lesion-wise counts and metrics
def lesion_counts(pred, gt, C, connectivity=8, overlap=(0, 1), min_px=None, label=label_flood):
    """int64 [B, C, 4] = (n_gt, n_gt_hit, n_pred, n_pred_hit).  pred is labelled over the pixels gt does not ignore; inter of a component =
    its pixels with pred == gt that lie in a component on both sides; hit iff inter >= 1 and inter t_den >= t_num area; components with
    area < min_px[b] are not counted on their side (their pixels still overlap the other side's)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    t_num, t_den = overlap
    assert 0 <= t_num <= t_den and 0 < t_den < 1 << 20
    pc, pa, _ = label(pred, C, connectivity, gt)
    gc, ga, _ = label(gt, C, connectivity, None)
    B, H, W = pred.shape
    counts = np.zeros((B, C, 4), np.int64)
    for b in range(B):
        mp = 1 if min_px is None else int(min_px[b])
        both = (pc[b] >= 0) & (gc[b] >= 0) & (pred[b] == gt[b])
        for side, (comp, area, lab) in enumerate(((gc[b], ga[b], gt[b]), (pc[b], pa[b], pred[b]))):
            inter = np.bincount(comp[both].ravel(), minlength=H * W)
            for r in np.flatnonzero(area.ravel() > 0):
                a = int(area.ravel()[r])
                if a < mp:
                    continue
                c = int(lab.ravel()[r])
                counts[b, c, 2 * side] += 1
                n = int(inter[r])
                if n >= 1 and n * t_den >= t_num * a:
                    counts[b, c, 2 * side + 1] += 1
    return counts


def lesion_metrics(counts, images=None):
    """Sums over images; per class sensitivity, precision, F1, false positives per image as float64 (NaN where the denominator is 0)."""
    counts = np.asarray(counts)
    if counts.ndim == 3:
        images = counts.shape[0] if images is None else images
        counts = counts.sum(0)
    n_gt, gt_hit, n_pred, pred_hit = (counts[:, i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        sens = np.where(n_gt > 0, gt_hit / n_gt, np.nan)
        prec = np.where(n_pred > 0, pred_hit / n_pred, np.nan)
        f1 = np.where(prec + sens > 0, 2 * prec * sens / (prec + sens), np.nan)
        fp = (n_pred - pred_hit) / images if images > 0 else np.full_like(n_gt, np.nan)
    return {"sensitivity": sens, "precision": prec, "f1": f1, "fp_per_image": fp, "n_gt": counts[:, 0], "n_gt_hit": counts[:, 1],
            "n_pred": counts[:, 2], "n_pred_hit": counts[:, 3], "images": images}


def min_px(min_area_mm2, spacing):
    """ceil(min_area_mm2 / (s_y s_x)) per image in float64."""
    return [int(np.ceil(np.float64(min_area_mm2) / (np.float64(s[0]) * np.float64(s[1])))) for s in spacing]
