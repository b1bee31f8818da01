#!/usr/bin/env python3
"""Time of the boundary-loss kernels (csrc/distmap.hip, the boundary variants of csrc/segloss.hip), by the method of tools/cc_bench.py:
whole ``ops`` calls between HIP events, five windows of back-to-back calls after a warm-up, each at least MIN_S seconds; median with min
and max.

  * ops.signed_distance_map at B = 8, C = 3 on blob maps (three classes cut from smoothed noise, four ignored columns) at 224^2 and
    1024^2, beside ops.surface_stats on the same maps (the project's yardstick for a label-map kernel) and the single-threaded
    scipy.ndimage route on the host (one timed pass; left out where scipy is missing);
  * ops.seg_loss_bd_fwd + seg_loss_bd_bwd against ops.seg_loss_fwd + seg_loss_bwd at B = 32, g = 14, u = 16, C = 3.

A library without the boundary entry points (an older build given through DINOX_LIB) is timed on the old calls alone: that is the A/B of
the untouched kernels.  The timing runs in a child process under its own time limit, so a hang ends the tool instead of holding the
device; the parent never opens the GPU.  One JSON line at the end.

    python tools/bdloss_bench.py            [ROUNDS=5 MIN_S=0.2 SIZES=224,1024 TIMEOUT=420]
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
SIZES = [int(s) for s in os.environ.get("SIZES", "224,1024").split(",")]
TIMEOUT = int(os.environ.get("TIMEOUT", 420))
B, C = 8, 3
LB, LG, LU = 32, 14, 16


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


def blob_maps(torch, S, g):
    noise = torch.rand((B, 1, S, S), device="cuda", generator=g)
    k = max(S // 14, 3) | 1
    smooth = torch.nn.functional.avg_pool2d(noise, k, stride=1, padding=k // 2, count_include_pad=False)[:, 0]
    cuts = torch.quantile(smooth.flatten()[:1 << 20], torch.tensor([0.6, 0.85], device="cuda"))
    gt = torch.bucketize(smooth, cuts).to(torch.uint8)
    pred = torch.roll(gt, (2, 3), (1, 2)).clone()
    gt[:, :, :4] = 255
    return pred, gt


def scipy_ms(gt, spacing):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    y, sp = gt.cpu().numpy(), spacing.cpu().numpy().astype("float64")
    t0 = time.perf_counter()
    for b in range(B):
        for c in range(C):
            G = y[b] == c
            _ = ndi.distance_transform_edt(~G, sampling=sp[b]) * ~G - ndi.distance_transform_edt(G, sampling=sp[b]) * G
    return (time.perf_counter() - t0) * 1e3


def report(torch, row, name, call):
    ts = [timed(torch, call, MIN_S) for _ in range(ROUNDS)]
    row[name] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
    print(f"{row['what']:28s} {name:22s} {row[name]['ms']:9.4f} ms (min {row[name]['min_ms']:.4f}, max {row[name]['max_ms']:.4f})", flush=True)


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    torch.set_num_threads(1)                                # the scipy route is the single-threaded one
    from dinox import _lib, ops
    assert torch.cuda.is_available(), "bdloss_bench needs a GPU"
    have_bd = hasattr(_lib.lib, "dinox_signed_distance") and hasattr(ops, "signed_distance_map")
    g = torch.Generator(device="cuda").manual_seed(0)
    spacing = torch.tensor([[0.8, 1.3]], device="cuda").repeat(B, 1)
    results = []
    for S in SIZES if have_bd else []:
        pred, gt = blob_maps(torch, S, g)
        row = {"what": f"maps B={B} C={C} {S}x{S}"}
        report(torch, row, "signed_distance_map", lambda: ops.signed_distance_map(gt, spacing, C))
        report(torch, row, "surface_stats", lambda: ops.surface_stats(pred, gt, spacing, C))
        ms = scipy_ms(gt, spacing)
        if ms is not None:
            row["scipy_edt_1_thread"] = {"ms": round(ms, 2)}
            print(f"{row['what']:28s} {'scipy edt, 1 thread':22s} {ms:9.2f} ms (one pass, 2 transforms per plane)", flush=True)
        results.append(row)
    Sl = LG * LU
    z = torch.randn((LB, LG * LG, C), device="cuda", generator=g) * 3
    y = blob_maps(torch, Sl, g)[1].repeat(LB // B, 1, 1)
    row = {"what": f"loss B={LB} g={LG} u={LU} C={C}"}

    def old():
        return ops.seg_loss_bwd(ops.seg_loss_fwd(z, y, 1.0, 1.0, 0)[2])

    report(torch, row, "seg_loss fwd+bwd", old)
    if have_bd:
        phi = ops.signed_distance_map(y, torch.ones((LB, 2), device="cuda"), C)

        def new():
            return ops.seg_loss_bd_bwd(ops.seg_loss_bd_fwd(z, y, phi, 1.0, 1.0, 0.5, 0)[2])

        report(torch, row, "seg_loss_bd fwd+bwd", new)
        report(torch, row, "signed_distance_map", lambda: ops.signed_distance_map(y, torch.ones((LB, 2), device="cuda"), C))
    results.append(row)
    print(json.dumps({"tool": "bdloss_bench", "library": os.path.basename(_lib.LIB_PATH), "rounds": ROUNDS, "min_s": MIN_S, "results": results}))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"bdloss_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
