#!/usr/bin/env python3
"""Micro-benchmark of the probe block: dinox_gram_f32 (csrc/gram.hip), dinox_softmax_probe (csrc/probe.hip) and the whole logistic fit
of dinox.probes, at the evaluation's scale (N = 65 536 unit rows, D = 384, C = 8 datasets).

Both kernels read x once, so HBM is the roof: the GB/s printed are bytes of x over the median time.  Candidates ALTERNATE inside one
process (ROUNDS rounds, each timed for at least MIN_S seconds between HIP events, after a warm-up); medians and the spread
(max - min) / median are printed.  Then the whole fit (wall clock, with its evaluation count) and the three metrics end to end, and --
when scikit-learn imports -- the same three computations the reference's way on the host (LogisticRegression(max_iter=1000), Ridge,
SVD statistics, on OMP_NUM_THREADS host threads); "n/a" otherwise.  One JSON line at the end.

    python tools/probe_bench.py            [ROUNDS=5 MIN_S=0.2 N=65536 D=384 C=8]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dino-x_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dinox import ops, probes  # noqa: E402

ROUNDS = int(os.environ.get("ROUNDS", 5))
MIN_S = float(os.environ.get("MIN_S", 0.2))
N, D, C = (int(os.environ.get(k, v)) for k, v in (("N", 65536), ("D", 384), ("C", 8)))
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


def main():
    g = torch.Generator(device=dev).manual_seed(0)
    label = torch.randint(0, C, (N,), device=dev, generator=g)
    centre = torch.randn(C, D, device=dev, generator=g)
    E = ops.normalize_rows(0.35 * centre[label] + torch.randn(N, D, device=dev, generator=g))[0]
    theta = 0.5 * torch.randn(C, D + 1, device=dev, generator=g)
    shift = E.mean(0)
    names = [f"dataset_{int(c)}" for c in label.cpu()]
    series = [f"{names[i]}/series_{i // 64:05d}" for i in range(N)]
    sx = np.exp(np.random.default_rng(0).uniform(np.log(0.45), np.log(1.0), N // 64 + 1))[np.arange(N) // 64]
    spacings = np.stack([sx, sx, np.full_like(sx, 2.5)], 1)

    cands = {
        "gram": lambda: ops.gram(E),
        "gram_shifted": lambda: ops.gram(E, shift),
        "softmax_probe": lambda: ops.softmax_probe(E, label, theta, want_grad=True),
        "softmax_probe_predict": lambda: ops.softmax_probe(E, label, theta, want_grad=False, want_prob=True),
    }
    times = {k: [] for k in cands}
    for fn in cands.values():
        fn()
    for _ in range(ROUNDS):
        for k, fn in cands.items():
            times[k].append(timed(fn, MIN_S))
    result = {"N": N, "D": D, "C": C, "rounds": ROUNDS}
    gb = N * D * 4 / 1e9
    print(f"N = {N}, D = {D}, C = {C}; x is {gb * 1e3:.1f} MB; medians of {ROUNDS} interleaved rounds")
    for k, v in times.items():
        med = statistics.median(v)
        result[k] = {"us": med * 1e3, "gbps": gb / (med * 1e-3), "spread": (max(v) - min(v)) / med}
        print(f"  {k:24s} {med * 1e3:9.1f} us   {gb / (med * 1e-3):8.1f} GB/s of x   spread {(max(v) - min(v)) / med:.3f}")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    wall(lambda: probes.logistic_probe(E, names, series, return_details=True))          # warm-up
    fits = [wall(lambda: probes.logistic_probe(E, names, series, return_details=True)) for _ in range(3)]
    out, ms = sorted(fits, key=lambda f: f[1])[1]
    result["logistic_probe"] = {"ms": ms, "evaluations": out["fit"]["evaluations"], "stopped_by": out["fit"]["stopped_by"], "accuracy": out["accuracy"]}
    print(f"  logistic_probe (split, fit, predict, bootstrap)  {ms:9.1f} ms   {out['fit']['evaluations']} evaluations, stopped by "
          f"{out['fit']['stopped_by']}, accuracy {out['accuracy']:.4f}")
    for name, fn in (("spacing_ridge", lambda: probes.spacing_ridge(E, spacings, names, series)),
                     ("embedding_stats", lambda: probes.embedding_stats(E, spacings, names))):
        fn()
        ms = statistics.median(wall(fn)[1] for _ in range(3))
        result[name] = {"ms": ms}
        print(f"  {name:48s} {ms:9.1f} ms")

    try:
        from sklearn.linear_model import LogisticRegression, Ridge
    except Exception:
        print("  scikit-learn route: n/a (not installed here)")
        result["sklearn"] = "n/a"
    else:
        X, y = E.cpu().numpy(), label.cpu().numpy()
        sp = probes.series_split(names, series, 42)
        t0 = time.perf_counter()
        LogisticRegression(max_iter=1000, random_state=42, solver="lbfgs").fit(X[sp.train_idx], y[sp.train_idx]).predict_proba(X[sp.test_idx])
        t1 = time.perf_counter()
        Ridge(alpha=1.0).fit(X[sp.train_idx], np.log(sx[sp.train_idx] + 1e-6)).predict(X[sp.test_idx])
        t2 = time.perf_counter()
        for c in range(C):
            e = X[y == c]
            np.linalg.svd(e - e.mean(0), full_matrices=False)
        t3 = time.perf_counter()
        result["sklearn"] = {"logistic_ms": (t1 - t0) * 1e3, "ridge_ms": (t2 - t1) * 1e3, "stats_svd_ms": (t3 - t2) * 1e3}
        threads = os.environ.get("OMP_NUM_THREADS") or len(os.sched_getaffinity(0))
        print(f"  host route (scikit-learn / NumPy, {threads} threads): logistic {(t1 - t0) * 1e3:.0f} ms, ridge "
              f"{(t2 - t1) * 1e3:.0f} ms, per-dataset SVD {(t3 - t2) * 1e3:.0f} ms")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
