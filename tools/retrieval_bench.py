#!/usr/bin/env python3
"""Micro-benchmark of dinox_retrieval_rank (csrc/retrieval.hip) against the yardstick it replaces: dinox_gemm in fp32 mode writing the
materialised similarity matrix S = Q K^T at the same shape (gemm_f32_big, the same exact-fp32 MFMA).

Shapes: N = 4096, 16 384, 65 536 at D = 384 and N = 16 384 at D = 1024; unit rows.  Per shape the two kernels ALTERNATE inside one
process (ROUNDS rounds, each candidate timed for at least MIN_S seconds per round between HIP events, after a warm-up).  The GEMM runs
only where S fits comfortably (N <= 16 384: 1 GiB).  Printed per shape: median time, fp32 TFLOP/s from 2 Nq Nk D, share of the 157.3 TF
fp32 matrix peak (the kernel is compute-bound: q and k are at most 100 MB), the spread (max - min) / median over the rounds of each
candidate, and whether the fused kernel is within the GEMM's own spread of the GEMM.  One JSON line at the end.

    python tools/retrieval_bench.py            [ROUNDS=5 MIN_S=0.2 SHAPES=4096x384,16384x384]

``--groups G`` times the windowed entry instead (dinox_retrieval_rank_windowed, the per-dataset view retrieval of the pan-organ
evaluation): G groups of GROUP_ROWS (512) rows at D = GROUP_D (384), rows sorted by group, ONE windowed call over all G x 512 rows against
the loop of G dinox_retrieval_rank calls on the row slices -- what the evaluation would run without the windowed entry.  Same
alternation, rounds and median; the two must agree bit for bit (checked).

    python tools/retrieval_bench.py --groups 5     [ROUNDS=5 MIN_S=0.2 GROUP_ROWS=512 GROUP_D=384]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import torch  # noqa: E402

from dinox import ops  # noqa: E402

PEAK_TF = 157.3
ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "4096x384,16384x384,65536x384,16384x1024").split(",")]
GEMM_MAX_N = 16384
dev = "cuda"


def timed(fn, min_s):
    """Time per launch (ms): HIP events around one window of back-to-back launches lasting at least min_s seconds."""
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


def groups_main(G):
    n, D = int(os.environ.get("GROUP_ROWS", 512)), int(os.environ.get("GROUP_D", 384))
    N = G * n
    g = torch.Generator(device=dev).manual_seed(0)
    q = ops.normalize_rows(torch.randn(N, D, device=dev, generator=g))[0]
    k = ops.normalize_rows(q + 0.5 * torch.randn(N, D, device=dev, generator=g))[0]
    key_lo = (torch.arange(N, device=dev) // n * n).to(torch.int32)
    key_hi = key_lo + n
    slices = [(q[a:a + n], k[a:a + n]) for a in range(0, N, n)]
    cands = {"windowed": lambda: ops.retrieval_rank_windowed(q, k, key_lo, key_hi),
             "loop_of_rank_calls": lambda: [ops.retrieval_rank(a, b) for a, b in slices]}
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    one, many = cands["windowed"](), cands["loop_of_rank_calls"]()
    same = all(torch.equal(one[o].view(torch.int32), torch.cat([m[o] for m in many]).view(torch.int32)) for o in (0, 2, 3)) and \
        torch.equal(one[1], torch.cat([m[1] + i * n for i, m in enumerate(many)]))
    times = {name: [] for name in cands}
    for _ in range(ROUNDS):
        for name, fn in cands.items():
            times[name].append(timed(fn, MIN_S))
    row = {"groups": G, "rows_per_group": n, "D": D, "bitwise_equal": bool(same)}
    for name, ts in times.items():
        med = statistics.median(ts)
        row[name] = {"ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "spread": round((max(ts) - min(ts)) / med, 4)}
        print(f"G={G:3d} n={n} D={D} {name:20s} {med:10.4f} ms  spread {100 * row[name]['spread']:.2f} %", flush=True)
    row["windowed_over_loop"] = round(row["windowed"]["ms"] / row["loop_of_rank_calls"]["ms"], 4)
    print(f"         windowed / loop = {row['windowed_over_loop']:.4f}  bitwise equal: {same}", flush=True)
    print(json.dumps({"tool": "retrieval_bench", "mode": "groups", "rounds": ROUNDS, "min_s": MIN_S, "results": [row]}))


def main():
    assert torch.cuda.is_available(), "retrieval_bench needs a GPU"
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=0, metavar="G", help="time the windowed call against a loop of G per-group calls")
    args = ap.parse_args()
    if args.groups > 0:
        return groups_main(args.groups)
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for N, D in SHAPES:
        q = ops.normalize_rows(torch.randn(N, D, device=dev, generator=g))[0]
        k = ops.normalize_rows(q + 0.5 * torch.randn(N, D, device=dev, generator=g))[0]
        flops = 2.0 * N * N * D
        cands = {"retrieval_rank": lambda: ops.retrieval_rank(q, k)}
        S = None
        if N <= GEMM_MAX_N:
            S = torch.empty(N, N, dtype=torch.float32, device=dev)
            cands["gemm_f32_S"] = lambda: ops.gemm(q, k, out=S)
        for fn in cands.values():                                   # warm-up of every shape the timed windows use
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(ROUNDS):
            for name, fn in cands.items():                          # alternate inside one process
                times[name].append(timed(fn, MIN_S))
        row = {"N": N, "D": D}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name] = {"ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                         "spread": round((max(ts) - min(ts)) / med, 4), "tflops": round(flops / med / 1e9, 2),
                         "share_of_fp32_matrix_peak": round(flops / med / 1e9 / PEAK_TF, 4)}
        if S is not None:
            r, y = row["retrieval_rank"], row["gemm_f32_S"]
            row["fused_over_gemm"] = round(r["ms"] / y["ms"], 4)
            row["within_gemm_spread"] = bool(r["ms"] <= y["ms"] * (1.0 + y["spread"]))
            # the same products: the fused kernel's argmax must be an argmax of S up to fp32 ties
            _, bi, bv, _ = ops.retrieval_rank(q, k)
            ops.gemm(q, k, out=S)
            row["best_val_equals_rowmax_of_S"] = bool(torch.equal(bv, S.max(dim=1).values))
        results.append(row)
        for name in cands:
            c = row[name]
            print(f"N={N:6d} D={D:5d} {name:15s} {c['ms']:10.4f} ms  {c['tflops']:7.2f} TFLOP/s  {100 * c['share_of_fp32_matrix_peak']:5.1f} % of "
                  f"{PEAK_TF} TF  spread {100 * c['spread']:.2f} %", flush=True)
        if S is not None:
            print(f"         fused / gemm = {row['fused_over_gemm']:.4f}  within the GEMM's spread: {row['within_gemm_spread']}  "
                  f"best_val == rowmax(S) bitwise: {row['best_val_equals_rowmax_of_S']}", flush=True)
        del S, q, k
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "retrieval_bench", "rounds": ROUNDS, "min_s": MIN_S, "peak_tf": PEAK_TF, "results": results}))


if __name__ == "__main__":
    main()
