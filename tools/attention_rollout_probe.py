#!/usr/bin/env python3
"""Time the attention rollout against the plain forward it rides on, and dinox_attention_rollout_step on its own.

    python tools/attention_rollout_probe.py [--iters 20] [--rounds 3]

Models (random weights, eval, bf16 autocast): ViT-S/16 at 224 (B = 32, T = 201, 12 x 6 x 64) and ViT-L/14 at 518 (B = 1, T = 1374,
24 x 16 x 64).  Per model, `rounds` times alternately: `iters` plain `model(x)` calls, then `iters` `model.attention_rollout(x)` calls
(forward + one extra qkv product per block + the chain), each window between HIP events after a warm-up; milliseconds per call, host
launches included.  The forward's launches are not changed by the rollout code, so its figure is also the cost before the feature.
Then the step alone at both shapes with a dense w (every chunk of query rows does work: the steps after the first) and a one-hot w
(the first step: one chunk), microseconds per call, beside its cost model N^2 d fma per (image, head).  One line per case.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dino-x_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    import zoo.arch as arch
    from dinox import ops
    g = torch.Generator().manual_seed(0)
    models = [("vit-s/16@224", dict(img_size=224, patch=16, dim=384, depth=12, heads=6, num_registers=4), 32),
              ("vit-l/14@518", dict(img_size=518, patch=14, dim=1024, depth=24, heads=16, num_registers=4), 1)]
    for name, kw, B in models:
        torch.manual_seed(0)
        model = arch.PatchViT(**kw).cuda().eval()
        x = torch.randn(B, 3, kw["img_size"], kw["img_size"], generator=g).cuda()
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            fwd = lambda: model(x)
            roll = lambda: model.attention_rollout(x)
            for _ in range(3):
                fwd(), roll()
            torch.cuda.synchronize()
            for r in range(args.rounds):
                tf, tr = timed(fwd, args.iters), timed(roll, args.iters)
                print(f"rollout {name} B={B} bf16 round {r}: forward {tf:8.3f} ms   attention_rollout {tr:8.3f} ms   extra {tr - tf:8.3f} ms "
                      f"({kw['depth']} qkv products + {kw['depth']} steps)")
        del model
    for name, B, N, heads, d in (("vit-s/16@224", 32, 201, 6, 64), ("vit-l/14@518", 1, 1374, 16, 64)):
        qkv = torch.randn(B, N, 3 * heads * d, generator=g).to(torch.bfloat16).cuda()
        dense = torch.rand(B, N, generator=g).cuda()
        onehot = torch.zeros(B, N).cuda()
        onehot[:, 0] = 1.0
        for wname, w in (("dense", dense), ("one-hot", onehot)):
            fn = lambda: ops.attention_rollout_step(qkv, heads, w, 0.5)
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            for r in range(args.rounds):
                us = timed(fn, args.iters * 5) * 1e3
                print(f"attention_rollout_step {name} B={B} N={N} heads={heads} d={d} bf16 w={wname} round {r}: {us:9.1f} us per call "
                      f"(host launch and workspace allocation included)  model {N * N * d * B * heads / 1e6:8.1f} Mfma  workgroups {B * heads}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
