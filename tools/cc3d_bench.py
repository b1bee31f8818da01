#!/usr/bin/env python3
"""Time of ops.cc_label_3d, cc_filter_3d and lesion_counts_3d (csrc/cclabel3d.hip) on whole volumes, [256, 224, 224] and [128, 512, 512],
C = 3, each beside ops.cc_label on the same voxels taken as Z independent slices (csrc/cclabel.hip: the launches the volume path shares,
without the z links and with per-slice roots) -- the yardstick, and the ratio of the two.

Volumes: ``blobs`` (three classes cut from noise smoothed in all three directions, the prediction the labels shifted by (1, 2, 3) voxels with
2 % of the voxels re-drawn: large organs plus thousands of specks) and ``serpentine`` (in every even slice corridors on the even rows joined
at alternating ends, every odd slice one linking voxel at alternating ends of that path: one component that winds through every slice).
Timing as tools/cc_bench.py (its ``timed``): five windows of back-to-back calls between HIP events after a warm-up, each at least MIN_S
seconds; median with min and max; whole ``ops`` calls.  The timing runs in a child process under its own time limit.  One JSON line at the end.

    python tools/cc3d_bench.py            [ROUNDS=5 MIN_S=0.2 TIMEOUT=420]
"""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cc_bench import MIN_S, ROOT, ROUNDS, TIMEOUT, timed  # noqa: E402

SHAPES = ((256, 224, 224), (128, 512, 512))
C = 3


def make_volumes(torch, kind, shape, g):
    dev = "cuda"
    Z, H, W = shape
    if kind == "serpentine":
        plane = torch.zeros((H, W), dtype=torch.uint8, device=dev)
        plane[::2] = 1
        plane[1::4, W - 1] = 1
        plane[3::4, 0] = 1
        k = (H - 1) // 2
        far = (2 * k, W - 1 if k % 2 == 0 else 0)
        v = torch.zeros(shape, dtype=torch.uint8, device=dev)
        v[::2] = plane
        v[1::4, far[0], far[1]] = 1
        v[3::4, 0, 0] = 1
        gt = v.clone()
        gt[:, :, W // 2] = 0                        # the ground truth's corridors are cut in the middle
        return v, gt
    noise = torch.rand((1, 1, Z, H, W), device=dev, generator=g)
    k = max(H // 14, 3) | 1
    kz = max(min(Z // 14, k), 3) | 1
    smooth = noise
    for ks in ((kz, 1, 1), (1, k, 1), (1, 1, k)):  # a box filter, one direction at a time
        smooth = torch.nn.functional.avg_pool3d(smooth, ks, stride=1, padding=tuple(n // 2 for n in ks), count_include_pad=False)
    smooth = smooth[0, 0]
    cuts = torch.quantile(smooth.flatten()[:1 << 20], torch.tensor([0.6, 0.85], device=dev))
    gt = torch.bucketize(smooth, cuts).to(torch.uint8)
    pred = torch.roll(gt, (1, 2, 3), (0, 1, 2)).clone()
    redraw = torch.rand(shape, device=dev, generator=g) < 0.02
    pred[redraw] = torch.randint(0, C, (int(redraw.sum()),), device=dev, generator=g, dtype=torch.uint8)
    gt[:, :, :4] = 255
    return pred, gt


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dinox import ops
    assert torch.cuda.is_available(), "cc3d_bench needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for shape in SHAPES:
        for kind in ("blobs", "serpentine"):
            pred, gt = make_volumes(torch, kind, shape, g)
            calls = {"cc_label_3d_6": lambda: ops.cc_label_3d(pred, C, 6), "slices_cc_label_4": lambda: ops.cc_label(pred, C, 4),
                     "cc_label_3d_26": lambda: ops.cc_label_3d(pred, C, 26), "slices_cc_label_8": lambda: ops.cc_label(pred, C, 8),
                     "cc_filter_3d_26": lambda: ops.cc_filter_3d(pred, C, min_vox=20, keep_largest=True),
                     "slices_cc_filter_8": lambda: ops.cc_filter(pred, C, min_px=20, keep_largest=True),
                     "lesion_counts_3d_26": lambda: ops.lesion_counts_3d(pred, gt, C), "slices_lesion_counts_8": lambda: ops.lesion_counts(pred, gt, C)}
            row = {"shape": list(shape), "C": C, "volume": kind, "components_per_class": ops.cc_label_3d(pred, C, 26)[2].tolist(),
                   "components_per_class_slicewise": ops.cc_label(pred, C, 8)[2].sum(0).tolist()}
            tag = "x".join(map(str, shape))
            for name, call in calls.items():
                ts = [timed(torch, call, MIN_S) for _ in range(ROUNDS)]
                row[name] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
                print(f"{tag:12s} {kind:11s} {name:24s} {row[name]['ms']:9.4f} ms (min {row[name]['min_ms']:.4f}, max {row[name]['max_ms']:.4f})", flush=True)
            pairs = (("cc_label_3d_6", "slices_cc_label_4"), ("cc_label_3d_26", "slices_cc_label_8"), ("cc_filter_3d_26", "slices_cc_filter_8"),
                     ("lesion_counts_3d_26", "slices_lesion_counts_8"))
            row["ratio_3d_over_slices"] = {a: round(row[a]["ms"] / row[b]["ms"], 3) for a, b in pairs}
            print(f"{tag:12s} {kind:11s} 3-D / slice-wise: {row['ratio_3d_over_slices']}; components per class {row['components_per_class']} "
                  f"(slice-wise {row['components_per_class_slicewise']})", flush=True)
            results.append(row)
    print(json.dumps({"tool": "cc3d_bench", "rounds": ROUNDS, "min_s": MIN_S, "results": results}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"cc3d_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
