#!/usr/bin/env python3
"""Time of the edge-aware refinement (csrc/segrefine.hip, ops.seg_refine) by the method of tools/segblend_bench.py: whole calls between
HIP events, ROUNDS windows of back-to-back calls after a warm-up, each at least MIN_S seconds; median with min and max.

Shape: B = 64 slices of S = 224 (g = 14, u = 16), C = 8, the default window (r = 2, d = 2).  Rows: T = 0 (the first launch alone),
T = 1 and T = 5, so that (T5 - T1) / 4 is one full iteration (read a plane, write a plane), and ops.seg_predict for scale.  Beside the
times: the bytes one iteration must move (B C S^2 floats read and written once, the guide read once) and the rate that makes of them.
The workspace allocation of ops.seg_refine (torch's caching allocator) is inside the timed call, as a user pays it.

The timing runs in a child process under its own time limit; the parent never opens the GPU.  One JSON line at the end.

    python tools/segrefine_bench.py            [ROUNDS=5 MIN_S=0.2 TIMEOUT=300]
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
TIMEOUT = int(os.environ.get("TIMEOUT", 300))
B, G, U, C = 64, 14, 16, 8


def worker():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
    import torch
    from dinox import _lib, ops
    from segblend_bench import timed
    assert torch.cuda.is_available(), "segrefine_bench needs a GPU"
    S = G * U
    gen = torch.Generator(device="cuda").manual_seed(0)
    z = torch.randn((B, G * G, C), device="cuda", generator=gen) * 3
    guide = torch.randn((B, S, S), device="cuda", generator=gen)
    rows = {}
    fns = {"seg_predict": lambda: ops.seg_predict(z, U)}
    for T in (0, 1, 5):
        fns[f"seg_refine T={T}"] = lambda T=T: ops.seg_refine(z, guide, U, iters=T, want_conf=True)
    for name, fn in fns.items():
        ts = [timed(torch, fn, MIN_S) for _ in range(ROUNDS)]
        rows[name] = {"ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
        print(f"{name:18s} {rows[name]['ms']:9.4f} ms (min {rows[name]['min_ms']:.4f}, max {rows[name]['max_ms']:.4f})", flush=True)
    per_iter_ms = (rows["seg_refine T=5"]["ms"] - rows["seg_refine T=1"]["ms"]) / 4
    nbytes = 2 * B * C * S * S * 4 + B * S * S * 4
    out = {"tool": "segrefine_bench", "library": os.path.basename(_lib.LIB_PATH), "rounds": ROUNDS, "min_s": MIN_S,
           "what": f"B={B} S={S} C={C} r=2 d=2", "results": rows, "iteration_ms": round(per_iter_ms, 4), "iteration_bytes": nbytes,
           "iteration_gb_per_s": round(nbytes / (per_iter_ms * 1e-3) / 1e9, 1)}
    print(json.dumps(out))


def main():
    if "--worker" in sys.argv:
        return worker()
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], timeout=TIMEOUT).returncode
    except subprocess.TimeoutExpired:
        print(f"segrefine_bench: the timing step did not finish in {TIMEOUT} s", file=sys.stderr)
        rc = 124
    sys.exit(rc)


if __name__ == "__main__":
    main()
