#!/usr/bin/env python3
"""Time of one ops.surface_stats call (csrc/surfdist.hip) at B = 32, C = 4 for S = 224 and S = 512, and of the host route a user pays
without it.

Maps, per size: ``blobs`` (four classes cut from smoothed noise, the prediction the labels shifted by (2, 3) pixels with 2 % of the pixels
re-drawn: what a trained segmenter gives) and ``checkerboard`` (every pixel a border pixel of its class in both maps: the worst case of
the row minimum, what an early-epoch prediction looks like).  Five windows of back-to-back calls between HIP events after a warm-up, each
at least MIN_S seconds; median with min and max.  The host figure: the same maps copied to the host, per image and class
``binary_erosion`` for the two borders and ``scipy.ndimage.distance_transform_edt`` (sampling = the spacing) both ways, one pass over
the batch, single-threaded as scipy runs it; "missing" if scipy does not import.

The timing runs in a child process under its own time limit (TIMEOUT seconds), so a hang ends the tool instead of holding the device; the
parent never opens the GPU.  At most 16 host threads.  One JSON line at the end.

    python tools/surface_bench.py            [ROUNDS=5 MIN_S=0.2 SIZES=224,512 TIMEOUT=420]
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
SIZES = [int(v) for v in os.environ.get("SIZES", "224,512").split(",")]
TIMEOUT = int(os.environ.get("TIMEOUT", 420))
B, C = 32, 4
TOL = (1.0, 2.0)


def timed(torch, fn, min_s):
    """Time per call (ms): HIP events around one window of back-to-back calls lasting at least min_s seconds."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(2, int(min_s * 1e3 / max(a.elapsed_time(b), 1e-3)) + 1)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def make_maps(torch, S, kind, g):
    dev = "cuda"
    if kind == "checkerboard":
        y, x = torch.meshgrid(torch.arange(S, device=dev), torch.arange(S, device=dev), indexing="ij")
        pred = ((y + x) % C).to(torch.uint8).expand(B, S, S).contiguous()
        gt = ((y + 2 * x + 1) % C).to(torch.uint8).expand(B, S, S).contiguous()
        return pred, gt
    noise = torch.rand((B, 1, S, S), device=dev, generator=g)
    k = max(S // 14, 3) | 1
    smooth = torch.nn.functional.avg_pool2d(noise, k, stride=1, padding=k // 2, count_include_pad=False)[:, 0]
    cuts = torch.quantile(smooth.flatten()[:1 << 20], torch.tensor([0.55, 0.75, 0.9], device=dev))
    gt = torch.bucketize(smooth, cuts).to(torch.uint8)
    pred = torch.roll(gt, (2, 3), (1, 2)).clone()
    redraw = torch.rand((B, S, S), device=dev, generator=g) < 0.02
    pred[redraw] = torch.randint(0, C, (int(redraw.sum()),), device=dev, generator=g, dtype=torch.uint8)
    gt[:, :, :4] = 255
    return pred, gt


def host_route(pred, gt, spacing):
    """Seconds for the batch through scipy, or None."""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    p, g, sp = pred.cpu().numpy(), gt.cpu().numpy(), spacing.cpu().numpy()
    t0 = time.perf_counter()
    for b in range(p.shape[0]):
        for c in range(C):
            A, G = (g[b] != 255) & (p[b] == c), g[b] == c
            bA, bG = A & ~ndi.binary_erosion(A), G & ~ndi.binary_erosion(G)
            if bA.any() and bG.any():
                ndi.distance_transform_edt(~bG, sampling=tuple(sp[b]))[bA].sum()
                ndi.distance_transform_edt(~bA, sampling=tuple(sp[b]))[bG].sum()
    return time.perf_counter() - t0


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from dinox import _lib, ops
    assert torch.cuda.is_available(), "surface_bench needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for S in SIZES:
        spacing = 0.5 + torch.rand((B, 2), device="cuda", generator=g)
        for kind in ("blobs", "checkerboard"):
            pred, gt = make_maps(torch, S, kind, g)

            def call():
                return ops.surface_stats(pred, gt, spacing, C, tolerances=TOL)

            counts, _ = call()
            ts = [timed(torch, call, MIN_S) for _ in range(ROUNDS)]
            host = host_route(pred, gt, spacing)
            per_image = int(_lib.lib.dinox_surface_ws_bytes(1, S, S, C))
            row = {"S": S, "B": B, "C": C, "maps": kind, "ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4),
                   "max_ms": round(max(ts), 4), "border_pixels": int(counts[..., 0].sum()),
                   "images_per_call": max(1, min(B, ops.SURFACE_WS_CAP // per_image)), "ws_bytes_per_image": per_image,
                   "host_scipy_s": None if host is None else round(host, 3)}
            results.append(row)
            print(f"S={S:4d} {kind:12s} surface_stats {row['ms']:9.4f} ms (min {row['min_ms']:.4f}, max {row['max_ms']:.4f}), "
                  f"{row['border_pixels']} border pixels, {row['images_per_call']} images per call;  host scipy: "
                  + ("missing (scipy does not import)" if host is None else f"{host:.3f} s"), flush=True)
    print(json.dumps({"tool": "surface_bench", "rounds": ROUNDS, "min_s": MIN_S, "results": results}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"surface_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
