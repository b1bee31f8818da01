#!/usr/bin/env python3
"""Micro-benchmark of dinox_knn_topk (csrc/knn.hip) against its floor and against the framework route.

Operands: N clustered unit rows (64 clusters, x = c[label] + 0.7 n, as the float case of tests/test_knn_gpu.py) searched against
themselves, self excluded, in two layouts: ``shuffled`` (labels in random order) and ``by_cluster`` (rows stored cluster by cluster: the
unfriendly order for the threshold filter, a query's own cluster may come last).  Candidates, ALTERNATING inside one process (ROUNDS
rounds, each timed for at least MIN_S seconds per round between HIP events, after a warm-up):

  knn_topk K=10 / K=20   the kernel under test
  retrieval_rank         the same sweep without selection on the same operands: the floor
  torch_topk K=10        (Q @ K.T).topk(K) in fp32, chunked over the queries so that a chunk of S stays under CHUNK_MB; its peak
                         allocation is printed beside the kernel's workspace bytes

Printed per shape and layout: median time, exact-fp32 TFLOP/s from 2 N^2 D, spread (max - min) / median, knn / floor.  One JSON line
at the end.

    python tools/knn_bench.py            [ROUNDS=5 MIN_S=0.2 SHAPES=4096x384,16384x384,65536x384 CHUNK_MB=1024]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import torch  # noqa: E402

from dinox import _lib, ops  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
SHAPES = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SHAPES", "4096x384,16384x384,65536x384").split(",")]
CHUNK_MB = int(os.environ.get("CHUNK_MB", 1024))
KS = (10, 20)
dev = "cuda"


def timed(fn, min_s):
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


def clustered(N, D, g):
    c = torch.randn(64, D, device=dev, generator=g)
    label = torch.randint(0, 64, (N,), device=dev, generator=g)
    x = ops.normalize_rows(c[label] + 0.7 * torch.randn(N, D, device=dev, generator=g))[0]
    return x, label


def torch_topk(x, K, chunk):
    """The framework route: fp32 S chunk by chunk, diagonal masked, topk."""
    N = x.shape[0]
    idx = torch.empty(N, K, dtype=torch.int64, device=dev)
    val = torch.empty(N, K, dtype=torch.float32, device=dev)
    for lo in range(0, N, chunk):
        S = x[lo:lo + chunk] @ x.T
        S[torch.arange(S.shape[0], device=dev), torch.arange(lo, lo + S.shape[0], device=dev)] = float("-inf")
        val[lo:lo + chunk], idx[lo:lo + chunk] = S.topk(K, dim=1)
    return idx, val


def main():
    assert torch.cuda.is_available(), "knn_bench needs a GPU"
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device=dev).manual_seed(0)
    results = []
    for N, D in SHAPES:
        x0, label = clustered(N, D, g)
        flops = 2.0 * N * N * D
        chunk = max(1, min(N, CHUNK_MB * (1 << 20) // (4 * N)))
        for layout in ("shuffled", "by_cluster"):
            x = x0 if layout == "shuffled" else x0[torch.argsort(label, stable=True)].contiguous()
            cands = {f"knn_topk_K{K}": (lambda K=K: ops.knn_topk(x, x, K, exclude="self")) for K in KS}
            cands["retrieval_rank"] = lambda: ops.retrieval_rank(x, x)
            cands["torch_topk_K10"] = lambda: torch_topk(x, 10, chunk)
            for fn in cands.values():
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch_topk(x, 10, chunk)
            torch.cuda.synchronize()
            torch_peak = torch.cuda.max_memory_allocated() - base
            times = {name: [] for name in cands}
            for _ in range(ROUNDS):
                for name, fn in cands.items():                      # alternate inside one process
                    times[name].append(timed(fn, MIN_S))
            row = {"N": N, "D": D, "layout": layout, "torch_chunk_rows": chunk, "torch_peak_bytes": int(torch_peak),
                   "knn_ws_bytes": {f"K{K}": int(_lib.lib.dinox_knn_ws_bytes(N, N, D, K)) for K in KS}}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                             "spread": round((max(ts) - min(ts)) / med, 4), "tflops": round(flops / med / 1e9, 2)}
            for K in KS:
                row[f"knn_K{K}_over_floor"] = round(row[f"knn_topk_K{K}"]["ms"] / row["retrieval_rank"]["ms"], 4)
            # same neighbours as the framework route wherever its fp32 scores are not within 1e-5 of a tie at the K-th place
            i1, _ = ops.knn_topk(x, x, 10, exclude="self")
            i2, v2 = torch_topk(x, 11, chunk)
            clear = (v2[:, 9] - v2[:, 10]) > 1e-5
            row["rows_with_torch_neighbour_set"] = float((i1.long().sort(1).values[clear] == i2[:, :10].sort(1).values[clear]).all(1).float().mean())
            results.append(row)
            for name in cands:
                c = row[name]
                print(f"N={N:6d} D={D:4d} {layout:10s} {name:15s} {c['ms']:10.4f} ms  {c['tflops']:7.2f} TFLOP/s  spread {100 * c['spread']:.2f} %",
                      flush=True)
            print(f"         knn / floor: K=10 {row['knn_K10_over_floor']:.3f}, K=20 {row['knn_K20_over_floor']:.3f};  workspace "
                  f"{row['knn_ws_bytes']['K10'] / 2 ** 20:.1f} / {row['knn_ws_bytes']['K20'] / 2 ** 20:.1f} MiB, torch route peak "
                  f"{torch_peak / 2 ** 20:.1f} MiB ({chunk} query rows per chunk);  same neighbour set as torch on clear rows: "
                  f"{row['rows_with_torch_neighbour_set']:.4f}", flush=True)
            del x
        del x0
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "knn_bench", "rounds": ROUNDS, "min_s": MIN_S, "results": results}))


if __name__ == "__main__":
    main()
