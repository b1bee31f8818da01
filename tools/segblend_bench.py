#!/usr/bin/env python3
"""Time and peak memory of the tile-blend kernel (csrc/segblend.hip, ops.seg_blend_predict) against a plain-torch restatement on the same
GPU, by the method of tools/bdloss_bench.py: whole calls between HIP events, five windows of back-to-back calls after a warm-up, each at
least MIN_S seconds; median with min and max.  Peak memory: torch's allocator high-water mark over one call, above what was allocated
before it (inputs excluded, every temporary and the output included).

Shape: B = 16 images of 512 x 512, tiles of t = 224 at overlap 0.5 (4 x 4 origins), g = 14, C = 4, the four mirror variants, the Gaussian
window.  The torch restatement: F.interpolate (bilinear, align_corners=False) of every tile to [C, t, t], the mirror undone by flip, times
the window, index_add_ into [B, C, H W] and [H W] accumulators (index table built once, outside the timed region), division, arg-max.
Its index_add_ uses floating-point atomics, so unlike the kernel it is not bit-reproducible.  The share of pixels on which the two label
maps agree is reported beside the times.

The timing runs in a child process under its own time limit, so a hang ends the tool instead of holding the device; the parent never
opens the GPU.  One JSON line at the end.

    python tools/segblend_bench.py            [ROUNDS=5 MIN_S=0.2 TIMEOUT=420]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
TIMEOUT = int(os.environ.get("TIMEOUT", 420))
B, H, W, T, G, C, OVERLAP = 16, 512, 512, 224, 14, 4, 0.5
FLIPS = [0, 1, 2, 3]


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


def peak_mib(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 2)


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    import torch.nn.functional as F
    from dinox import _lib, ops
    from dinox.tiled import blend_window, tile_starts
    assert torch.cuda.is_available(), "segblend_bench needs a GPU"
    ys, xs, win = tile_starts(H, T, OVERLAP), tile_starts(W, T, OVERLAP), blend_window(T, "gaussian")
    ny, nx, nf = len(ys), len(xs), len(FLIPS)
    g = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn((B, nf, ny, nx, G * G, C), device="cuda", generator=g) * 3

    def native():
        return ops.seg_blend_predict(z, ys, xs, FLIPS, win, H, W, T)

    wt = torch.from_numpy(win).cuda()
    w2 = wt[:, None] * wt[None, :]                                                  # [t, t]
    ar = torch.arange(T, device="cuda")
    idx = torch.stack([((y0 + ar)[:, None] * W + (x0 + ar)[None, :]).reshape(-1) for y0 in ys for x0 in xs], 0)      # [ny nx, t t]
    idx_all = idx[None].expand(nf, -1, -1).reshape(-1)
    den = torch.zeros(H * W, device="cuda").index_add_(0, idx_all, w2.reshape(-1).repeat(nf * ny * nx))

    def plain():
        up = F.interpolate(z.view(-1, G, G, C).permute(0, 3, 1, 2), size=(T, T), mode="bilinear", align_corners=False)
        up = up.view(B, nf, ny * nx, C, T, T)
        parts = []
        for f, code in enumerate(FLIPS):
            dims = [d for d, bit in ((-1, 1), (-2, 2)) if code & bit]
            parts.append(up[:, f].flip(dims) if dims else up[:, f])
        vals = torch.stack(parts, 1) * w2                                           # [B, F, tiles, C, t, t]
        vals = vals.permute(0, 3, 1, 2, 4, 5).reshape(B, C, -1)
        acc = torch.zeros((B, C, H * W), device="cuda").index_add_(2, idx_all, vals)
        return (acc / den).argmax(1).to(torch.uint8).view(B, H, W)

    agree = float((native() == plain()).float().mean())
    row = {"what": f"B={B} {H}x{W} t={T} g={G} C={C} overlap={OVERLAP} F={nf} tiles={ny}x{nx}", "labels_agree": round(agree, 6)}
    for name, fn in (("native", native), ("torch", plain)):
        ts = [timed(torch, fn, MIN_S) for _ in range(ROUNDS)]
        row[name] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "peak_mib": peak_mib(torch, fn)}
        print(f"{name:8s} {row[name]['ms']:9.4f} ms (min {row[name]['min_ms']:.4f}, max {row[name]['max_ms']:.4f}), peak {row[name]['peak_mib']:.2f} MiB",
              flush=True)
    print(json.dumps({"tool": "segblend_bench", "library": os.path.basename(_lib.LIB_PATH), "rounds": ROUNDS, "min_s": MIN_S, "results": [row]}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"segblend_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
