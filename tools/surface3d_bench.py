#!/usr/bin/env python3
"""Time of one ops.surface_stats_3d call (csrc/surfdist3d.hip) on volumes of (64, 224, 224) and (256, 224, 224) voxels with C = 3, T = 2,
beside ops.surface_stats (csrc/surfdist.hip) on the same voxels taken as Z independent slices -- the same voxel count without the extra
axis -- and of the host route a user pays without either.

Maps, per size: ``blobs`` (three classes cut from noise smoothed in 3-D, the prediction the labels shifted by (1, 2, 3) voxels with 2 % of
the voxels re-drawn: what a trained segmenter gives) and ``checkerboard`` (every voxel a border voxel of its class in both volumes: the
worst case of the x minimum).  Five windows of back-to-back calls between HIP events after a warm-up, each at least MIN_S seconds; median
with min and max.  The host figure: the same volumes copied to the host, per class ``binary_erosion`` for the two borders and
``scipy.ndimage.distance_transform_edt`` (sampling = the voxel) both ways, single-threaded as scipy runs it; "missing" if scipy does not
import.

The timing runs in a child process under its own time limit (TIMEOUT seconds), so a hang ends the tool instead of holding the device; the
parent never opens the GPU.  At most 16 host threads.  One JSON line at the end.

    python tools/surface3d_bench.py            [ROUNDS=5 MIN_S=0.2 DEPTHS=64,256 TIMEOUT=420]
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from surface_bench import timed  # noqa: E402  (the same windows as the 2-D tool)

ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
DEPTHS = [int(v) for v in os.environ.get("DEPTHS", "64,256").split(",")]
TIMEOUT = int(os.environ.get("TIMEOUT", 420))
S, C = 224, 3
TOL = (1.0, 2.0)
VOXEL = (2.5, 0.7, 0.8)                             # (s_z, s_y, s_x) in mm


def make_maps(torch, Z, kind, g):
    dev = "cuda"
    if kind == "checkerboard":
        z, y, x = torch.meshgrid(torch.arange(Z, device=dev), torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
        return ((z + y + x) % C).to(torch.uint8).contiguous(), ((z + y + 2 * x + 1) % C).to(torch.uint8).contiguous()
    noise = torch.rand((1, 1, Z, S, S), device=dev, generator=g)
    smooth = torch.nn.functional.avg_pool3d(noise, (5, 17, 17), stride=1, padding=(2, 8, 8), count_include_pad=False)[0, 0]
    cuts = torch.quantile(smooth.flatten()[:1 << 20], torch.tensor([0.7, 0.9], device=dev))
    gt = torch.bucketize(smooth, cuts).to(torch.uint8)
    pred = torch.roll(gt, (1, 2, 3), (0, 1, 2)).clone()
    redraw = torch.rand((Z, S, S), device=dev, generator=g) < 0.02
    pred[redraw] = torch.randint(0, C, (int(redraw.sum()),), device=dev, generator=g, dtype=torch.uint8)
    gt[:, :, :4] = 255
    return pred, gt


def host_route(pred, gt):
    """Seconds for the volume through scipy, or None."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    p, g = pred.cpu().numpy(), gt.cpu().numpy()
    t0 = time.perf_counter()
    for c in range(C):
        A, G = (g != 255) & (p == c), g == c
        bA, bG = A & ~ndi.binary_erosion(A), G & ~ndi.binary_erosion(G)
        if bA.any() and bG.any():
            ndi.distance_transform_edt(~bG, sampling=VOXEL)[bA].sum()
            ndi.distance_transform_edt(~bA, sampling=VOXEL)[bG].sum()
    return time.perf_counter() - t0


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dinox import _lib, ops
    assert torch.cuda.is_available(), "surface3d_bench needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for Z in DEPTHS:
        plane = torch.tensor([VOXEL[1:]] * Z, device="cuda")
        for kind in ("blobs", "checkerboard"):
            pred, gt = make_maps(torch, Z, kind, g)
            counts, _ = ops.surface_stats_3d(pred, gt, VOXEL, C, tolerances=TOL)
            t3 = [timed(torch, lambda: ops.surface_stats_3d(pred, gt, VOXEL, C, tolerances=TOL), MIN_S) for _ in range(ROUNDS)]
            t2 = [timed(torch, lambda: ops.surface_stats(pred, gt, plane, C, tolerances=TOL), MIN_S) for _ in range(ROUNDS)]
            host = host_route(pred, gt)
            m3, m2 = statistics.median(t3), statistics.median(t2)
            row = {"Z": Z, "H": S, "W": S, "C": C, "maps": kind, "ms_3d": round(m3, 4), "min_ms_3d": round(min(t3), 4), "max_ms_3d": round(max(t3), 4),
                   "ms_slices_2d": round(m2, 4), "min_ms_slices_2d": round(min(t2), 4), "max_ms_slices_2d": round(max(t2), 4),
                   "ratio_3d_over_slices": round(m3 / m2, 3), "border_voxels": int(counts[:, :, 0].sum()),
                   "ws_bytes": int(_lib.lib.dinox_surface3d_ws_bytes(Z, S, S, C)), "host_scipy_s": None if host is None else round(host, 3)}
            results.append(row)
            print(f"({Z:3d}, {S}, {S}) {kind:12s} surface_stats_3d {m3:9.4f} ms (min {min(t3):.4f}, max {max(t3):.4f});  surface_stats on the Z slices "
                  f"{m2:9.4f} ms (min {min(t2):.4f}, max {max(t2):.4f});  3-D / slice-wise {m3 / m2:.2f};  {row['border_voxels']} border voxels;  "
                  "host scipy: " + ("missing (scipy does not import)" if host is None else f"{host:.3f} s"), flush=True)
    print(json.dumps({"tool": "surface3d_bench", "rounds": ROUNDS, "min_s": MIN_S, "voxel_mm": VOXEL, "results": results}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"surface3d_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
